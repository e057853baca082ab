// model_host.h -- the host-side driver the model forwards share (vit.hip, eva.hip, ccip.hip, convnext.hip, swinv2.hip): checkpoint
// upload helpers, the ledger of tensors still to be set, input staging / read-back and the sub-batch fork / join.  Host code only,
// everything inline or a template; a model file adds its kernels, its kernel sequence and its own rule for the number of sub-batches.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "vit_internal.h"

namespace hipts {

inline int upload_f32(DevBuf& buf, const float* data, size_t n) {
    HIPTS_TRY(buf.alloc(n * 4));
    return upload(buf.p, data, n * 4);
}

// [W | W / lo_scale] as 16-bit operands: the weight of a GEMM whose A operand arrives as (hi | lo * lo_scale) halves (K = 2 cols)
inline int upload_matrix16_dup(DevBuf& buf, const float* data, int rows, int cols, int rows_pad, bool f16, float lo_scale = 1.0f) {
    std::vector<float> dup((size_t)rows * 2 * cols);
    const float inv = 1.0f / lo_scale;
    for (int n = 0; n < rows; ++n) {
        const float* src = data + (size_t)n * cols;
        float* dst = &dup[(size_t)n * 2 * cols];
        memcpy(dst, src, (size_t)cols * 4);
        if (lo_scale == 1.0f) memcpy(dst + cols, src, (size_t)cols * 4);
        else for (int k = 0; k < cols; ++k) dst[cols + k] = src[k] * inv;
    }
    return upload_matrix16(buf, dup.data(), rows, 2 * cols, rows_pad, f16);
}

// Stem / patch-embedding convolution weight [n][3][taps] -> [n][t * 3 + c_mem], written twice: at columns 0 and kh of a 2 kh wide row
// (against the hi | lo halves of the patch matrix; pad columns zero).  bgr: memory channel c_mem reads model channel 2 - c_mem.
inline std::vector<float> stem_weight_hilo(const float* data, int n_out, int taps, int kh, bool bgr) {
    std::vector<float> w2((size_t)n_out * 2 * kh, 0.f);
    for (int n = 0; n < n_out; ++n)
        for (int cm = 0; cm < 3; ++cm)
            for (int t = 0; t < taps; ++t) {
                const float v = data[((size_t)n * 3 + (bgr ? 2 - cm : cm)) * taps + t];
                w2[(size_t)n * 2 * kh + t * 3 + cm] = v;
                w2[(size_t)n * 2 * kh + kh + t * 3 + cm] = v;
            }
    return w2;
}

// ToTensor + Normalize of a byte, tabulated [3][256]: u / 255 in float32, (x - mean) / std in T (float: timm's transform; double:
// gen_cfeatures.py's numpy arithmetic), stored float32
template <typename T>
inline std::vector<float> norm_lut(const T* mean, const T* stdv) {
    std::vector<float> lut(3 * 256);
    for (int c = 0; c < 3; ++c)
        for (int u = 0; u < 256; ++u) lut[c * 256 + u] = (float)(((T)((float)u / 255.0f) - mean[c]) / stdv[c]);
    return lut;
}

// The checkpoint tensors a handle still waits for, in the order they were asked for.
struct TensorLedger {
    std::vector<std::string> missing;
    void need(const std::string& key) { missing.push_back(key); }
    void mark_set(const std::string& key) {
        auto it = std::find(missing.begin(), missing.end(), key);
        if (it != missing.end()) missing.erase(it);
    }
    int require_complete(const char* fn) const {
        if (missing.empty()) return HIPTS_OK;
        return set_error(HIPTS_ERR_STATE, "%s: %zu checkpoint tensors not set (first: %s)", fn, missing.size(), missing[0].c_str());
    }
};

// "<prefix><index>.<rest>" -> index, rest; false when s does not have that form
inline bool parse_indexed(const std::string& s, const char* prefix, int* index, std::string* rest) {
    const size_t n = strlen(prefix);
    if (s.rfind(prefix, 0) != 0) return false;
    const size_t dot = s.find('.', n);
    if (dot == std::string::npos) return false;
    *index = atoi(s.substr(n, dot - n).c_str());
    *rest = s.substr(dot + 1);
    return true;
}

// in a set_tensor function (its arguments key_c and numel in scope)
#define EXPECT_NUMEL(n)                                                                                                \
    do {                                                                                                               \
        if (numel != (int64_t)(n))                                                                                     \
            return ::hipts::set_error(HIPTS_ERR_INVALID, "tensor %s: %lld elements, expected %lld", key_c, (long long)numel, (long long)(n)); \
    } while (0)

// kernel<F16> on the operand type: <true> first, as the sources always had it (the order of instantiation is the order of the
// kernels in the code object)
#define HIPTS_LAUNCH_F16(f16, kernel, grid, block, lds, stream, ...)                           \
    do {                                                                                       \
        if (f16) kernel<true><<<grid, block, lds, stream>>>(__VA_ARGS__);                      \
        else kernel<false><<<grid, block, lds, stream>>>(__VA_ARGS__);                         \
        HIPTS_LAUNCH_CHECK();                                                                  \
    } while (0)

// kernel<F16>(from_u8 or from_f32, ...) on the input type and the operand type, for a kernel whose first argument is the policy that
// reads the images (patch_rows.h).  Four instantiations in the order the sources always had them: uint8 input with half, then bf16
// operands, then float32 input with half, then bf16
#define HIPTS_LAUNCH_U8_F16(is_u8, f16, kernel, grid, block, lds, stream, from_u8, from_f32, ...)    \
    do {                                                                                       \
        if (is_u8) {                                                                           \
            if (f16) kernel<true><<<grid, block, lds, stream>>>(from_u8, __VA_ARGS__);         \
            else kernel<false><<<grid, block, lds, stream>>>(from_u8, __VA_ARGS__);            \
        } else {                                                                               \
            if (f16) kernel<true><<<grid, block, lds, stream>>>(from_f32, __VA_ARGS__);        \
            else kernel<false><<<grid, block, lds, stream>>>(from_f32, __VA_ARGS__);           \
        }                                                                                      \
        HIPTS_LAUNCH_CHECK();                                                                  \
    } while (0)

// a GEMM launch's arguments with the two fields every launch of a forward sets alike
inline GemmArgs gemm_args(bool f16, bool shared_chip) {
    GemmArgs g{};
    g.f16 = f16;
    g.shared_chip = shared_chip;
    return g;
}

// Internal streams and events of the sub-batch split.  Nothing is created before the first split forward: a handle that only sees
// small batches opens no stream of its own (a process has few hardware queues).  Destroyed with the handle, whose destroy function
// has synchronised the device before.
template <int N>
struct SubStreams {
    hipStream_t sub[N] = {};
    hipEvent_t ev_fork = nullptr, ev_join[N] = {};
    SubStreams() = default;
    SubStreams(const SubStreams&) = delete;
    SubStreams& operator=(const SubStreams&) = delete;
    ~SubStreams() {
        for (int i = 0; i < N; ++i) {
            if (sub[i]) (void)hipStreamDestroy(sub[i]);
            if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
        }
        if (ev_fork) (void)hipEventDestroy(ev_fork);
    }
    int ensure() {
        if (ev_fork) return HIPTS_OK;
        HIPTS_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
        for (int i = 0; i < N; ++i) {
            HIPTS_HIP(hipStreamCreateWithFlags(&sub[i], hipStreamNonBlocking));
            HIPTS_HIP(hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming));
        }
        return HIPTS_OK;
    }
};

// *in_dev = the images on the device: `input` itself, or its copy in img_in (grow-only) ordered on s
inline int stage_input(DevBuf& img_in, const void* input, int memspace, size_t bytes, hipStream_t s, const void** in_dev) {
    *in_dev = input;
    if (memspace == HIPTS_DEVICE) return HIPTS_OK;
    HIPTS_TRY(img_in.reserve(bytes));
    HIPTS_HIP(hipMemcpyAsync(img_in.p, input, bytes, hipMemcpyHostToDevice, s));
    *in_dev = img_in.p;
    return HIPTS_OK;
}

// up to two host outputs of `bytes` each (a null one is skipped), then the stream is drained
inline int read_back(hipStream_t s, size_t bytes, void* out0, const void* dev0, void* out1 = nullptr, const void* dev1 = nullptr) {
    if (out0) HIPTS_HIP(hipMemcpyAsync(out0, dev0, bytes, hipMemcpyDeviceToHost, s));
    if (out1) HIPTS_HIP(hipMemcpyAsync(out1, dev1, bytes, hipMemcpyDeviceToHost, s));
    HIPTS_HIP(hipStreamSynchronize(s));
    return HIPTS_OK;
}

// run(first image, images, stream, shared_chip, sub-batch index) for the whole batch on s (ns < 2), or for ns sub-batches on the internal
// streams, forked from s and joined back into it.  Two sub-batches: the larger half first; more: batch * i / ns.  The split changes
// which images share a launch, never an image's arithmetic.  (The ViT forward keeps a loop of its own: deferred join, stagger.)
template <int N, typename F>
int run_split(SubStreams<N>& ss, hipStream_t s, int batch, int ns, F&& run) {
    if (ns < 2) return run(0, batch, s, false, 0);
    HIPTS_TRY(ss.ensure());
    HIPTS_HIP(hipEventRecord(ss.ev_fork, s));
    for (int i = 0; i < ns; ++i) {
        const int a0 = ns == 2 ? (i ? (batch + 1) / 2 : 0) : (int)((int64_t)batch * i / ns);
        const int a1 = ns == 2 ? (i ? batch : (batch + 1) / 2) : (int)((int64_t)batch * (i + 1) / ns);
        HIPTS_HIP(hipStreamWaitEvent(ss.sub[i], ss.ev_fork, 0));
        HIPTS_TRY(run(a0, a1 - a0, ss.sub[i], true, i));
        HIPTS_HIP(hipEventRecord(ss.ev_join[i], ss.sub[i]));
        HIPTS_HIP(hipStreamWaitEvent(s, ss.ev_join[i], 0));
    }
    return HIPTS_OK;
}

}  // namespace hipts
