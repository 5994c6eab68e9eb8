// weight_fp8.hip -- the FP8 (OCP e4m3fn) form of the packed linear weight the drafter's stream-K GEMMs read (drafter_fc.hip,
// linear_rows_streamk_kernel<.., W8 = true>): weight-only, one f32 scale per output row.
//   s[n]   = max_k |W[n, k]| / 448 (f32; 1 for an all-zero row)
//   q[n,k] = e4m3fn_rne(f32(W[n, k]) / s[n]), saturating at +-448 (no NaN code is ever written)
// Layout: the brick sequence of lantern_pack_linear_weight -- one brick per (32-row tile, 64-element K block, set), gate / up pairs interleaved per
// brick, rows padded to a multiple of 32 with zero rows -- one byte per element, 2 KB per brick:
//   brick[j * 1024 + lane * 16 + e] = q[set * pair_rows + tile * 32 + (lane & 31)][kb * 64 + 32 (lane >> 5) + 16 j + e]      (j < 2, e < 16)
// i.e. a lane's 16 bytes of half j are its B-fragment elements of MFMA steps 2j and 2j + 1 (8 each), and a wave's 16-byte load is 1 KB contiguous.
// Behind the bricks: the f32 scales, scale[set * n_pad + n] for the n_pad = 32 * tiles padded rows of each set (1 for the padding rows).
#include "common.h"
#include "fp8_dev.h"          // f32_to_e4m3fn

namespace lantern {

// pass 1: one workgroup per padded row of every set -> its scale
__global__ __launch_bounds__(256) void fp8_row_scale_kernel(const uint16_t *__restrict__ W, int n_rows, int n_pad, int K, int pair_rows, float *__restrict__ scale) {
    __shared__ uint32_t red[4];
    const int set = blockIdx.x / n_pad, row = blockIdx.x % n_pad, tid = threadIdx.x;
    uint32_t m = 0;          // |bf16| bits order like the values
    if (row < n_rows) {
        const uint16_t *wr = W + (size_t)(set * pair_rows + row) * K;
        for (int i = tid * 8; i < K; i += 256 * 8) {
            const uint4 v = *reinterpret_cast<const uint4 *>(wr + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t lo = w[c] & 0x7fffu, hi = (w[c] >> 16) & 0x7fffu;
                m = m > lo ? m : lo;
                m = m > hi ? m : hi;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)m, o, 64);
        m = m > other ? m : other;
    }
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) m = m > red[w] ? m : red[w];
        scale[blockIdx.x] = m == 0 ? 1.0f : bf16_bits_to_f32((uint16_t)m) / 448.0f;
    }
}

// pass 2: one thread per 16 output bytes
__global__ void pack_linear_weight_fp8_kernel(const uint16_t *__restrict__ W, int n_rows, int n_pad, int K, int sets, int pair_rows, const float *__restrict__ scale,
                                              uint8_t *__restrict__ out, long long n_frag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frag) return;
    const int lane = (int)(i & 63), j = (int)((i >> 6) & 1);
    long long b = i >> 7;
    const int set = (int)(b % sets);
    b /= sets;
    const int kb = (int)(b % (K / 64)), tile = (int)(b / (K / 64));
    const int row = tile * 32 + (lane & 31);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    if (row < n_rows) {
        const float s = scale[set * n_pad + row];
        const uint16_t *src = W + (size_t)(set * pair_rows + row) * K + kb * 64 + 32 * (lane >> 5) + 16 * j;
        const uint4 v0 = *reinterpret_cast<const uint4 *>(src), v1 = *reinterpret_cast<const uint4 *>(src + 8);
        const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t lo = f32_to_e4m3fn(bf16_bits_to_f32((uint16_t)(w[c] & 0xffffu)) / s);
            const uint32_t hi = f32_to_e4m3fn(bf16_bits_to_f32((uint16_t)(w[c] >> 16)) / s);
            o[c >> 1] |= (lo | (hi << 8)) << (16 * (c & 1));
        }
    }
    reinterpret_cast<uint4 *>(out)[i] = make_uint4(o[0], o[1], o[2], o[3]);
}

// bricks -> row-major codes [N, K] (N = n_rows, or 2 * pair_rows ... rows set * pair_rows + n) and scales [N]
__global__ void unpack_linear_weight_fp8_kernel(const uint8_t *__restrict__ packed, int n_rows, int n_pad, int K, int sets, int pair_rows, uint8_t *__restrict__ q_out,
                                                float *__restrict__ scale_out, long long n_frag) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_frag) return;
    const int lane = (int)(i & 63), j = (int)((i >> 6) & 1);
    long long b = i >> 7;
    const int set = (int)(b % sets);
    b /= sets;
    const int kb = (int)(b % (K / 64)), tile = (int)(b / (K / 64));
    const int row = tile * 32 + (lane & 31);
    if (row >= n_rows) return;
    const size_t orow = (size_t)set * pair_rows + row;
    *reinterpret_cast<uint4 *>(q_out + orow * K + kb * 64 + 32 * (lane >> 5) + 16 * j) = reinterpret_cast<const uint4 *>(packed)[i];
    if (kb == 0 && j == 0 && (lane >> 5) == 0) scale_out[orow] = reinterpret_cast<const float *>(packed + (size_t)n_pad * K * sets)[set * n_pad + row];
}

}  // namespace lantern

using namespace lantern;

extern "C" size_t lantern_pack_linear_weight_fp8_bytes(int n_rows, int K, int pair_rows) {
    if (n_rows <= 0 || K <= 0 || K % 64) return 0;
    const size_t n_pad = (size_t)((n_rows + 31) / 32) * 32, sets = pair_rows > 0 ? 2 : 1;
    return n_pad * (size_t)K * sets + n_pad * sets * sizeof(float);
}

extern "C" int lantern_pack_linear_weight_fp8(const void *W, int n_rows, int K, int pair_rows, void *out, void *stream) {
    LANTERN_CHECK_ARG(W && out && n_rows > 0 && K > 0 && pair_rows >= 0, "pack_linear_weight_fp8: null buffer or bad sizes");
    if (K % 64 != 0) {
        set_error("pack_linear_weight_fp8: K=%d must be a multiple of 64 (the brick's K block)", K);
        return LANTERN_E_UNSUPPORTED;
    }
    LANTERN_CHECK_ARG(((uintptr_t)W & 15) == 0 && ((uintptr_t)out & 15) == 0, "pack_linear_weight_fp8: W and out must be 16-byte aligned");
    const int sets = pair_rows > 0 ? 2 : 1, n_pad = (n_rows + 31) / 32 * 32;
    float *scale = reinterpret_cast<float *>((uint8_t *)out + (size_t)n_pad * K * sets);
    hipLaunchKernelGGL(fp8_row_scale_kernel, dim3((unsigned)(n_pad * sets)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)W, n_rows, n_pad, K, pair_rows, scale);
    LANTERN_CHECK_LAUNCH("pack_linear_weight_fp8 (row scales)");
    const long long n_frag = (long long)(n_pad / 32) * (K / 64) * sets * 128;
    hipLaunchKernelGGL(pack_linear_weight_fp8_kernel, dim3((unsigned)((n_frag + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)W, n_rows, n_pad, K, sets,
                       pair_rows, scale, (uint8_t *)out, n_frag);
    LANTERN_CHECK_LAUNCH("pack_linear_weight_fp8");
    return LANTERN_OK;
}

extern "C" int lantern_unpack_linear_weight_fp8(const void *packed, int n_rows, int K, int pair_rows, uint8_t *q_out, float *scale_out, void *stream) {
    LANTERN_CHECK_ARG(packed && q_out && scale_out && n_rows > 0 && K > 0 && pair_rows >= 0, "unpack_linear_weight_fp8: null buffer or bad sizes");
    if (K % 64 != 0) {
        set_error("unpack_linear_weight_fp8: K=%d must be a multiple of 64 (the brick's K block)", K);
        return LANTERN_E_UNSUPPORTED;
    }
    LANTERN_CHECK_ARG(((uintptr_t)packed & 15) == 0 && ((uintptr_t)q_out & 15) == 0, "unpack_linear_weight_fp8: packed and q_out must be 16-byte aligned");
    const int sets = pair_rows > 0 ? 2 : 1, n_pad = (n_rows + 31) / 32 * 32;
    const long long n_frag = (long long)(n_pad / 32) * (K / 64) * sets * 128;
    hipLaunchKernelGGL(unpack_linear_weight_fp8_kernel, dim3((unsigned)((n_frag + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)packed, n_rows, n_pad, K,
                       sets, pair_rows, q_out, scale_out, n_frag);
    LANTERN_CHECK_LAUNCH("unpack_linear_weight_fp8");
    return LANTERN_OK;
}
