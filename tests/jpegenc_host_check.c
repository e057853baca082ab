/* Stand-alone memory-safety check of the host coder (csrc/jpeg_host.c: hipts_jpeg_entropy_encode), built by
 * tests/test_jpegenc_reference.py with -fsanitize=address,undefined together with jpeg_host.c and run on the CPU.
 *
 *     jpegenc_host_check SLOT FILE [SLOT FILE ...]
 *
 * Every SLOT (a coefficient slot, csrc/jpeg_slot.h) is coded into a heap buffer of exactly the size of FILE and must give FILE's bytes;
 * the file is decoded back into a heap buffer of exactly the slot's size and must give the slot.  Then the refusals, each on heap copies
 * of exactly the sizes passed, so that a read or a store one byte out of bounds is the sanitizer's to report: a bad magic, 4:4:4
 * sampling, an offset beyond slot_bytes, a coefficient of 2048, a slot cut short, and every capacity from one byte short down to
 * nothing.  Prints "ok" and exits 0 when all of it holds. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "jpeg_slot.h"

int hipts_jpeg_entropy_encode(const void* slot, int64_t slot_bytes, uint8_t* file_out, int64_t capacity, int64_t* nbytes);
int hipts_jpeg_entropy_decode(const uint8_t* data, int64_t n, void* slot, int64_t slot_bytes);

static uint8_t* read_file(const char* path, int64_t* n) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    *n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* p = malloc((size_t)*n);
    if (fread(p, 1, (size_t)*n, f) != (size_t)*n) exit(2);
    fclose(f);
    return p;
}

#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                  \
        }                                                              \
    } while (0)

/* the status of coding a changed copy of the slot into a buffer that would hold the file */
static int refused(const uint8_t* slot, int64_t slot_bytes, int64_t file_bytes, void (*change)(uint8_t*)) {
    uint8_t* s = malloc((size_t)slot_bytes);
    uint8_t* out = malloc((size_t)file_bytes);
    memcpy(s, slot, (size_t)slot_bytes);
    change(s);
    int64_t nb = -1;
    const int st = hipts_jpeg_entropy_encode(s, slot_bytes, out, file_bytes, &nb);
    free(s);
    free(out);
    return nb == 0 ? st : -1;
}

static void bad_magic(uint8_t* s) { s[0] ^= 1; }
static void sampling_444(uint8_t* s) {
    hipts_jpeg_header* h = (hipts_jpeg_header*)s;
    h->hmax = h->vmax = h->comp[0].h = h->comp[0].v = 1;
}
static void offset_beyond(uint8_t* s) { ((hipts_jpeg_header*)s)->comp[2].offset += 64; }
static void coefficient_2048(uint8_t* s) { ((int16_t*)(s + HIPTS_JPEG_HEADER_BYTES))[0] = 2048; }
static void ac_1024(uint8_t* s) { ((int16_t*)(s + HIPTS_JPEG_HEADER_BYTES))[64 + 9] = -1024; }

int main(int argc, char** argv) {
    if (argc < 3 || (argc & 1) == 0) return 2;
    for (int a = 1; a + 1 < argc; a += 2) {
        int64_t slot_bytes, file_bytes, nb = -1;
        uint8_t* slot = read_file(argv[a], &slot_bytes);
        uint8_t* want = read_file(argv[a + 1], &file_bytes);
        uint8_t* out = malloc((size_t)file_bytes);
        CHECK(hipts_jpeg_entropy_encode(slot, slot_bytes, out, file_bytes, &nb) == 0);
        CHECK(nb == file_bytes && memcmp(out, want, (size_t)nb) == 0);
        uint8_t* back = malloc((size_t)slot_bytes);
        memset(back, 0xA5, (size_t)slot_bytes);
        CHECK(hipts_jpeg_entropy_decode(out, nb, back, slot_bytes) == 0);
        CHECK(memcmp(back, slot, (size_t)slot_bytes) == 0);
        free(back);

        CHECK(refused(slot, slot_bytes, file_bytes, bad_magic) == 3);
        CHECK(refused(slot, slot_bytes, file_bytes, sampling_444) == 1);
        CHECK(refused(slot, slot_bytes, file_bytes, offset_beyond) == 3);
        CHECK(refused(slot, slot_bytes, file_bytes, coefficient_2048) == 3);
        CHECK(refused(slot, slot_bytes, file_bytes, ac_1024) == 3);
        /* the slot cut short: the header still promises all of it */
        {
            uint8_t* s = malloc((size_t)slot_bytes - 2);
            memcpy(s, slot, (size_t)slot_bytes - 2);
            CHECK(hipts_jpeg_entropy_encode(s, slot_bytes - 2, out, file_bytes, &nb) == 3 && nb == 0);
            free(s);
            s = malloc(100);
            memcpy(s, slot, 100);
            CHECK(hipts_jpeg_entropy_encode(s, 100, out, file_bytes, &nb) == 2 && nb == 0);
            free(s);
        }
        /* every capacity that is too small, in a buffer of exactly that size */
        for (int64_t cap = file_bytes - 1; cap >= 0; cap -= (cap > 700 ? 37 : 1)) {
            uint8_t* small = malloc((size_t)cap + 1); /* (malloc(0) may return NULL) */
            uint8_t* exact = realloc(small, (size_t)(cap ? cap : 1));
            nb = -1;
            CHECK(hipts_jpeg_entropy_encode(slot, slot_bytes, exact, cap, &nb) == 2 && nb == 0);
            free(exact);
        }
        free(out);
        free(want);
        free(slot);
    }
    puts("ok");
    return 0;
}
