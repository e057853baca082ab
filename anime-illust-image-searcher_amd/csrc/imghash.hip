// imghash.hip -- a 128-bit gradient hash of the model-input tensor (hipts_image_hash_u8): which FILES hold the same picture?
//
// Goes past the reference, which cannot list the re-saves, rescales and second downloads of a picture.  The definition (restated from
// include/hip_tagsearch.h; tests/imghash_ref.py is the numpy statement of it), all of it integer arithmetic:
//   grey     per pixel, Pillow's convert("L"):  g = (19595 R + 38470 G + 7471 B + 0x8000) >> 16
//   grids    a grid of Rr rows x Cc columns has the boundaries floor(k * size / Rr) and floor(k * size / Cc); sum(r, c) is the integer sum
//            of g over a cell, area(r, c) its pixel count (unequal whenever 9 does not divide size)
//   brighter cell b is brighter than cell a when  sum(b) * area(a) > sum(a) * area(b)  in 64-bit integers: the means compared exactly
//   word 0   grid 8 x 9: bit 8 r + c (r, c in 0..7) is set when cell (r, c + 1) is brighter than cell (r, c)
//   word 1   grid 9 x 8: bit 8 r + c is set when cell (r + 1, c) is brighter than cell (r, c)
// The comparison is strict: a flat region sets no bits.
//
//   imghash_bins_kernel    the sums of g over the common refinement of the two grids: both axes are cut at every floor(k size / 8) and
//                          floor(k size / 9), at most 16 bands each.  A workgroup takes a run of rows of one image; a thread takes 16
//                          consecutive pixels of a row -- three 16-byte loads where size is a multiple of 16 and the images are 16-byte
//                          aligned, byte loads otherwise --, sums g while the column band stays the same and adds each run to the
//                          workgroup's 16 x 16 bins in LDS; the non-zero bins then go to the image's bins in global memory with integer
//                          atomics.  Integer adds only: any order gives the same bits, and no workgroup waits for another one.
//   imghash_finish_kernel  one workgroup per image: the 72 + 72 cell sums out of the bins (a cell is a run of at most three bands on either
//                          axis), the 128 comparisons, one ballot per word.
// Algorithmic traffic: 3 size^2 bytes read per image (38.5 MB for 64 images at 448), 1 KiB of bins and 16 bytes of hash per image.
#include <algorithm>
#include <cstdlib>

#include "common.h"

using namespace hipts;

namespace {

constexpr int IH_MIN_SIZE = 9, IH_MAX_SIZE = 1024;
constexpr int IH_BANDS = 16;                 // bands per axis of the common refinement, at most
constexpr int IH_THREADS = 256;
constexpr int IH_RUN = 16;                   // pixels per thread and step: 48 bytes

struct HashGrid {
    int32_t bound[IH_BANDS + 1];             // band b is [bound[b], bound[b + 1]); entries past nb hold size
    int32_t nb;
};

HashGrid make_grid(int size) {
    HashGrid g;
    int cuts[18], n = 0;
    for (int k = 0; k <= 8; ++k) cuts[n++] = (int)((int64_t)k * size / 8);
    for (int k = 0; k <= 9; ++k) cuts[n++] = (int)((int64_t)k * size / 9);
    std::sort(cuts, cuts + n);
    n = (int)(std::unique(cuts, cuts + n) - cuts);               // size >= 9: the cuts of either grid are distinct, 0 and size shared
    g.nb = n - 1;
    for (int b = 0; b <= IH_BANDS; ++b) g.bound[b] = b < n ? cuts[b] : size;
    return g;
}

// VEC: size is a multiple of 16 and the images are 16-byte aligned -- every run of 16 pixels is three aligned 16-byte pieces
template <bool VEC>
__global__ __launch_bounds__(IH_THREADS) void imghash_bins_kernel(const uint8_t* __restrict__ images, int size, int split, int rows_per, HashGrid G,
                                                                  uint32_t* __restrict__ bins_out) {
    __shared__ uint32_t bins[IH_BANDS * IH_BANDS];
    __shared__ __attribute__((aligned(16))) uint8_t band[IH_MAX_SIZE + IH_RUN];      // band of a row or column index
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x / split;
    const int part = blockIdx.x % split;
    bins[tid] = 0;
    for (int x = tid; x < size + IH_RUN; x += IH_THREADS) {
        int b = 0;
#pragma unroll
        for (int k = 1; k < IH_BANDS; ++k) b += (k < G.nb && x >= G.bound[k]) ? 1 : 0;
        band[x] = (uint8_t)b;
    }
    __syncthreads();
    const int y0 = part * rows_per, y1 = min(size, y0 + rows_per);
    const int runs = (size + IH_RUN - 1) / IH_RUN;                 // per row
    const uint8_t* __restrict__ base = images + img * size * size * 3;
    for (int item = tid; item < (y1 - y0) * runs; item += IH_THREADS) {
        const int y = y0 + item / runs, x0 = (item % runs) * IH_RUN;
        const uint8_t* __restrict__ p = base + ((int64_t)y * size + x0) * 3;
        uint32_t w[12];                                            // 48 bytes = 16 pixels, bytes past the row are zero
        if (VEC) {
            const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1], c = reinterpret_cast<const uint4*>(p)[2];
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
        } else {
            const int nbytes = min(IH_RUN, size - x0) * 3;
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                uint32_t v = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (4 * k + q < nbytes) v |= (uint32_t)p[4 * k + q] << (8 * q);
                w[k] = v;
            }
        }
        const int npix = min(IH_RUN, size - x0);
        const uint4 cb4 = *reinterpret_cast<const uint4*>(&band[x0]);
        const uint32_t cbw[4] = {cb4.x, cb4.y, cb4.z, cb4.w};
        uint32_t* __restrict__ row = &bins[(int)band[y] * IH_BANDS];
        int cur = (int)(cbw[0] & 255u);
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < IH_RUN; ++i) {
            auto byte_at = [&](int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; };
            const uint32_t g = (19595u * byte_at(3 * i) + 38470u * byte_at(3 * i + 1) + 7471u * byte_at(3 * i + 2) + 0x8000u) >> 16;
            const int cb = (int)((cbw[i >> 2] >> (8 * (i & 3))) & 255u);
            if (i < npix) {
                if (cb != cur) {                                   // the bands ascend along the row: a run of 16 pixels meets a few
                    atomicAdd(&row[cur], acc);
                    acc = 0;
                    cur = cb;
                }
                acc += g;
            }
        }
        atomicAdd(&row[cur], acc);
    }
    __syncthreads();
    const uint32_t v = bins[tid];
    if (v) atomicAdd(&bins_out[img * (IH_BANDS * IH_BANDS) + tid], v);          // an image's sum is at most 255 * 1024^2 < 2^32
}

__global__ __launch_bounds__(IH_THREADS) void imghash_finish_kernel(const uint32_t* __restrict__ bins_in, int size, HashGrid G,
                                                                    unsigned long long* __restrict__ hashes) {
    __shared__ uint32_t bins[IH_BANDS * IH_BANDS];
    __shared__ uint32_t cell[2][72];                               // word 0: [r][c] of the 8 x 9 grid; word 1: [r][c] of the 9 x 8 grid
    const int tid = threadIdx.x;
    const int64_t img = blockIdx.x;
    bins[tid] = bins_in[img * (IH_BANDS * IH_BANDS) + tid];
    __syncthreads();
    if (tid < 144) {
        const int word = tid / 72, k = tid % 72;
        const int rows = word ? 9 : 8, cols = word ? 8 : 9;
        const int r = k / cols, c = k % cols;
        // a cell is a run of bands on either axis: the band that starts at a cut x is the number of bounds 1 .. nb that are <= x
        auto band_at = [&](int x) {
            int b = 0;
#pragma unroll
            for (int i = 1; i <= IH_BANDS; ++i) b += (i <= G.nb && x >= G.bound[i]) ? 1 : 0;
            return b;
        };
        auto cut = [&](int i, int parts) { return (int)((int64_t)i * size / parts); };
        const int r0 = band_at(cut(r, rows)), r1 = band_at(cut(r + 1, rows)), c0 = band_at(cut(c, cols)), c1 = band_at(cut(c + 1, cols));
        uint32_t s = 0;
        for (int rb = r0; rb < r1; ++rb)
            for (int cb = c0; cb < c1; ++cb) s += bins[rb * IH_BANDS + cb];
        cell[word][k] = s;
    }
    __syncthreads();
    if (tid < 128) {                                               // wave 0: word 0, wave 1: word 1; lane = bit
        const int word = tid >> 6, bit = tid & 63;
        const int r = bit >> 3, c = bit & 7;
        const int rows = word ? 9 : 8, cols = word ? 8 : 9;
        const int r2 = word ? r + 1 : r, c2 = word ? c : c + 1;    // the neighbour below, or to the right
        auto extent = [&](int k, int parts) { return (int)((int64_t)(k + 1) * size / parts) - (int)((int64_t)k * size / parts); };
        const unsigned long long area_a = (unsigned long long)extent(r, rows) * extent(c, cols);
        const unsigned long long area_b = (unsigned long long)extent(r2, rows) * extent(c2, cols);
        const unsigned long long sum_a = cell[word][r * cols + c], sum_b = cell[word][r2 * cols + c2];
        const unsigned long long m = __ballot(sum_b * area_a > sum_a * area_b);      // at most 255 * 2^14 * 2^14: exact in 64 bits
        if (bit == 0) hashes[img * 2 + word] = m;
    }
}

// Handle-less entry point: its workspace is kept per device and shared by every caller, ordered by an event (as the resize's temporary)
struct HashState {
    std::mutex mu;
    DevBuf stage[64], bins[64], out[64];
    hipEvent_t last[64] = {};
};
HashState& state() {
    static HashState* s = new HashState;         // never destroyed: the runtime may be gone before static destructors run
    return *s;
}

// Workgroups per image.  Default: enough of them to give every CU about four; HIPTS_IMGHASH_SPLIT sets it for a measurement
// (tools/dedup_bench.py, profiles/dedup.txt).
int split_for(int batch, int size) {
    const char* e = getenv("HIPTS_IMGHASH_SPLIT");
    int64_t split = e && *e ? atoll(e) : ((int64_t)4 * current_device_cus() + batch - 1) / batch;
    return (int)std::max<int64_t>(1, std::min<int64_t>(split, size));
}

}  // namespace

extern "C" int hipts_image_hash_u8(const uint8_t* images, int images_memspace, int batch, int size, uint64_t* hashes_out, int out_memspace,
                                   int device, void* stream) {
    HIPTS_REQUIRE(images && hashes_out, "hipts_image_hash_u8: null argument");
    HIPTS_REQUIRE(batch >= 1, "hipts_image_hash_u8: batch must be at least 1, got %d", batch);
    HIPTS_REQUIRE(size >= IH_MIN_SIZE && size <= IH_MAX_SIZE, "hipts_image_hash_u8: size must be in [%d, %d], got %d", IH_MIN_SIZE, IH_MAX_SIZE,
                  size);
    HIPTS_REQUIRE(device >= 0 && device < 64, "hipts_image_hash_u8: device index");
    HIPTS_TRY(use_device(device));
    hipStream_t s = (hipStream_t)stream;
    HashState& st = state();
    std::lock_guard<std::mutex> lock(st.mu);
    if (st.last[device]) HIPTS_HIP(hipStreamWaitEvent(s, st.last[device], 0));
    else HIPTS_HIP(hipEventCreateWithFlags(&st.last[device], hipEventDisableTiming));
    const size_t image_bytes = (size_t)size * size * 3, bins_bytes = (size_t)batch * IH_BANDS * IH_BANDS * 4;
    const bool host_in = images_memspace != HIPTS_DEVICE, host_out = out_memspace != HIPTS_DEVICE;
    const uint8_t* src = images;
    if (host_in) {
        HIPTS_TRY(st.stage[device].reserve((size_t)batch * image_bytes));
        HIPTS_HIP(hipMemcpyAsync(st.stage[device].p, images, (size_t)batch * image_bytes, hipMemcpyHostToDevice, s));
        src = st.stage[device].as<uint8_t>();
    }
    HIPTS_TRY(st.bins[device].reserve(bins_bytes));
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(hashes_out);
    if (host_out) {
        HIPTS_TRY(st.out[device].reserve((size_t)batch * 16));
        dst = st.out[device].as<unsigned long long>();
    }
    const HashGrid G = make_grid(size);
    const int split = split_for(batch, size);
    const int rows_per = (size + split - 1) / split;
    const int parts = (size + rows_per - 1) / rows_per;          // no empty workgroups
    const int64_t grid = (int64_t)batch * parts;
    HIPTS_REQUIRE(grid < ((int64_t)1 << 31), "hipts_image_hash_u8: batch %d is too large", batch);
    uint32_t* bins = st.bins[device].as<uint32_t>();
    HIPTS_HIP(hipMemsetAsync(bins, 0, bins_bytes, s));
    const bool vec = size % IH_RUN == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    if (vec) imghash_bins_kernel<true><<<(unsigned)grid, IH_THREADS, 0, s>>>(src, size, parts, rows_per, G, bins);
    else imghash_bins_kernel<false><<<(unsigned)grid, IH_THREADS, 0, s>>>(src, size, parts, rows_per, G, bins);
    HIPTS_LAUNCH_CHECK();
    imghash_finish_kernel<<<(unsigned)batch, IH_THREADS, 0, s>>>(bins, size, G, dst);
    HIPTS_LAUNCH_CHECK();
    if (host_out) HIPTS_HIP(hipMemcpyAsync(hashes_out, dst, (size_t)batch * 16, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipEventRecord(st.last[device], s));
    if (host_out) HIPTS_HIP(hipStreamSynchronize(s));
    return HIPTS_OK;
}
