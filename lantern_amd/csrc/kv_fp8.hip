// kv_fp8.hip -- the FP8 form of a KV-cache row (include/lantern_hip.h, "FP8 KV cache"): one key or value vector of one (batch row, kv head, position)
// is d + 16 bytes,
//   [0, d)        e4m3fn codes of the row's d elements
//   [d, d + 4)    the row's scale 2^e as an f32
//   [d + 4, d+16) zero, ignored by readers
// with e the smallest integer such that max|x| <= 448 * 2^e, clamped to [-64, 64] (0 for an all-zero row) and code = e4m3fn_rne(x / 2^e), saturating.
// The scale rides inside the row: a row stays a multiple of 16 bytes and the commit kernels (gather_ops.hip) move codes and scale together as an opaque
// row of elem_bytes = 1, d + 16 "elements".  code * 2^e is exactly a bf16 value, so the reader (tree_attention.hip, KV8) sees the dequantised cache.
//
// lantern_kv8_append: one row per D / 8 lanes (16 at d = 128, 8 at d = 64): a lane loads 16 bytes = 8 bf16 elements, the row maximum is taken inside
// the lane group with DPP moves (quad permutes, then the half-row / row mirrors), a lane makes its 8 code bytes, even lanes fetch their neighbour's 8
// with one more quad permute and store 16 bytes; lane 1 of the group stores the 16-byte tail.
#include "common.h"
#include "fp8_dev.h"

namespace lantern {

struct Kv8AppendArgs {
    const uint16_t *src[2];      // k_new / v_new (compacted: a NULL pair is left out)
    unsigned char *dst[2];       // k_cache / v_cache
    const int64_t *pos;
    int64_t pos0, S_max, n_sb, n_sh, n_st, kv_sb, kv_sh;
    int64_t n_rows;              // n_pairs * B * Hkv * T
    int B, Hkv, T;
};

template <int D>
__global__ __launch_bounds__(256) void kv8_append_kernel(const Kv8AppendArgs a) {
    constexpr int LPR = D / 8, RPB = 256 / LPR;
    const int tid = threadIdx.x, li = tid % LPR;
    const int64_t row = (int64_t)blockIdx.x * RPB + tid / LPR;
    // every lane stays active up to the stores (the DPP moves below read neighbours): `live` predicates the memory accesses only, and is uniform
    // over a row's lane group
    bool live = row < a.n_rows;
    const int64_t rr = live ? row : 0;
    const int t = (int)(rr % a.T), h = (int)((rr / a.T) % a.Hkv), b = (int)((rr / ((int64_t)a.T * a.Hkv)) % a.B);
    const int which = (int)(rr / ((int64_t)a.T * a.Hkv * a.B));
    const int64_t p = (a.pos ? a.pos[b] : a.pos0) + t;
    live = live && p >= 0 && p < a.S_max;          // a position outside the slab is skipped, never written
    uint4 x = make_uint4(0, 0, 0, 0);
    if (live) x = *reinterpret_cast<const uint4 *>(a.src[which] + (int64_t)b * a.n_sb + (int64_t)h * a.n_sh + (int64_t)t * a.n_st + 8 * li);
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    int m = 0;          // |bf16| bits order like the values
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        m = max(m, (int)(w[c] & 0x7fffu));
        m = max(m, (int)((w[c] >> 16) & 0x7fffu));
    }
    m = max(m, dpp_mov<0xB1>(m));                        // quad_perm [1,0,3,2]
    m = max(m, dpp_mov<0x4E>(m));                        // quad_perm [2,3,0,1]
    m = max(m, dpp_mov<0x141>(m));                       // row_half_mirror: the other quad of the 8 lanes
    if (D == 128) m = max(m, dpp_mov<0x140>(m));         // row_mirror: the other half of the 16 lanes
    // smallest e with amax <= 448 * 2^e = 1.75 * 2^(e + 8): amax = 1.f * 2^(E - 127) -> e = E - 135, one more when the fraction is above .75
    int e = m == 0 ? 0 : (m >> 7) - 135 + ((m & 0x7f) > 0x60 ? 1 : 0);
    e = e < KV8_EMIN ? KV8_EMIN : (e > KV8_EMAX ? KV8_EMAX : e);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);          // x * 2^-e = x / 2^e, exact
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const uint32_t lo = f32_to_e4m3fn(bf16_bits_to_f32((uint16_t)(w[c] & 0xffffu)) * inv);
        const uint32_t hi = f32_to_e4m3fn(bf16_bits_to_f32((uint16_t)(w[c] >> 16)) * inv);
        o[c >> 1] |= (lo | (hi << 8)) << (16 * (c & 1));
    }
    const uint32_t nx = (uint32_t)dpp_mov<0xB1>((int)o[0]), ny = (uint32_t)dpp_mov<0xB1>((int)o[1]);      // the odd neighbour's 8 codes
    if (!live) return;
    unsigned char *drow = a.dst[which] + (int64_t)b * a.kv_sb + (int64_t)h * a.kv_sh + p * (D + KV8_TAIL);
    if ((li & 1) == 0) *reinterpret_cast<uint4 *>(drow + 8 * li) = make_uint4(o[0], o[1], nx, ny);
    else if (li == 1) *reinterpret_cast<uint4 *>(drow + D) = make_uint4((uint32_t)(127 + e) << 23, 0u, 0u, 0u);
}

// one thread per 16 codes -> 16 bf16 values
template <int D>
__global__ __launch_bounds__(256) void kv8_dequantize_kernel(const unsigned char *__restrict__ cache, uint16_t *__restrict__ out, int64_t n_chunks) {
    constexpr int CPR8 = D / 16;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_chunks) return;
    const int64_t row = i / CPR8;
    const int ch = (int)(i % CPR8);
    const unsigned char *rp = cache + row * (D + KV8_TAIL);
    const uint4 c = *reinterpret_cast<const uint4 *>(rp + 16 * ch);
    const float s = *reinterpret_cast<const float *>(rp + D);
    uint16_t *op = out + row * D + 16 * ch;
    *reinterpret_cast<kv8_bf16x8_t *>(op) = kv8_expand8(make_uint2(c.x, c.y), s);
    *reinterpret_cast<kv8_bf16x8_t *>(op + 8) = kv8_expand8(make_uint2(c.z, c.w), s);
}

}  // namespace lantern

using namespace lantern;

extern "C" size_t lantern_kv8_row_bytes(int d) { return d == 64 || d == 128 ? (size_t)d + KV8_TAIL : 0; }

extern "C" int lantern_kv8_append(const void *k_new, const void *v_new, void *k_cache, void *v_cache, int B, int Hkv, int T, int d, int64_t new_stride_b,
                                  int64_t new_stride_h, int64_t new_stride_t, int64_t kv_stride_b_bytes, int64_t kv_stride_h_bytes, const int64_t *pos,
                                  int64_t pos0, int64_t S_max, void *stream) {
    if (d != 64 && d != 128) {
        set_error("kv8_append: head_dim %d not built (64 or 128)", d);
        return LANTERN_E_UNSUPPORTED;
    }
    LANTERN_CHECK_ARG((k_new != nullptr) == (k_cache != nullptr) && (v_new != nullptr) == (v_cache != nullptr) && (k_new || v_new),
                      "kv8_append: null pointer (k_new / k_cache and v_new / v_cache come in pairs, at least one pair)");
    LANTERN_CHECK_ARG(B >= 0 && Hkv > 0 && T >= 0 && S_max > 0, "kv8_append: bad sizes (B=%d Hkv=%d T=%d S_max=%lld)", B, Hkv, T, (long long)S_max);
    LANTERN_CHECK_ARG(new_stride_b % 8 == 0 && new_stride_h % 8 == 0 && new_stride_t % 8 == 0,
                      "kv8_append: strides of the new rows must be multiples of 8 elements (16-byte rows)");
    LANTERN_CHECK_ARG(kv_stride_b_bytes % 16 == 0 && kv_stride_h_bytes % 16 == 0, "kv8_append: cache byte strides must be multiples of 16");
    LANTERN_CHECK_ARG(kv_stride_h_bytes >= S_max * (d + KV8_TAIL), "kv8_append: kv_stride_h_bytes=%lld smaller than S_max*(d+16)",
                      (long long)kv_stride_h_bytes);
    LANTERN_CHECK_ARG(((uintptr_t)k_new | (uintptr_t)v_new | (uintptr_t)k_cache | (uintptr_t)v_cache) % 16 == 0, "kv8_append: pointers must be 16-byte aligned");
    LANTERN_CHECK_ARG(pos || pos0 >= 0, "kv8_append: pos0=%lld is negative", (long long)pos0);
    if (B == 0 || T == 0) return LANTERN_OK;
    Kv8AppendArgs a;
    int n = 0;
    a.src[1] = nullptr, a.dst[1] = nullptr;
    if (k_new) a.src[n] = (const uint16_t *)k_new, a.dst[n] = (unsigned char *)k_cache, ++n;
    if (v_new) a.src[n] = (const uint16_t *)v_new, a.dst[n] = (unsigned char *)v_cache, ++n;
    a.pos = pos, a.pos0 = pos0, a.S_max = S_max, a.n_sb = new_stride_b, a.n_sh = new_stride_h, a.n_st = new_stride_t;
    a.kv_sb = kv_stride_b_bytes, a.kv_sh = kv_stride_h_bytes, a.B = B, a.Hkv = Hkv, a.T = T;
    a.n_rows = (int64_t)n * B * Hkv * T;
    const int rpb = 256 / (d / 8);
    const int64_t blocks = (a.n_rows + rpb - 1) / rpb;
    LANTERN_CHECK_ARG(blocks < (1ll << 31), "kv8_append: %lld rows do not fit one launch", (long long)a.n_rows);
    if (d == 128) LANTERN_LAUNCH((kv8_append_kernel<128>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else LANTERN_LAUNCH((kv8_append_kernel<64>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    LANTERN_CHECK_LAUNCH("kv8_append");
    return LANTERN_OK;
}

extern "C" int lantern_kv8_dequantize(const void *cache, void *out_bf16, int64_t n_rows, int d, void *stream) {
    if (d != 64 && d != 128) {
        set_error("kv8_dequantize: head_dim %d not built (64 or 128)", d);
        return LANTERN_E_UNSUPPORTED;
    }
    LANTERN_CHECK_ARG(n_rows >= 0, "kv8_dequantize: n_rows=%lld", (long long)n_rows);
    if (n_rows == 0) return LANTERN_OK;
    LANTERN_CHECK_ARG(cache && out_bf16, "kv8_dequantize: null pointer");
    LANTERN_CHECK_ARG(((uintptr_t)cache | (uintptr_t)out_bf16) % 16 == 0, "kv8_dequantize: pointers must be 16-byte aligned");
    const int64_t n_chunks = n_rows * (d / 16), blocks = (n_chunks + 255) / 256;
    LANTERN_CHECK_ARG(blocks < (1ll << 31), "kv8_dequantize: %lld rows do not fit one launch", (long long)n_rows);
    if (d == 128) hipLaunchKernelGGL(kv8_dequantize_kernel<128>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char *)cache,
                                     (uint16_t *)out_bf16, n_chunks);
    else hipLaunchKernelGGL(kv8_dequantize_kernel<64>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned char *)cache,
                            (uint16_t *)out_bf16, n_chunks);
    LANTERN_CHECK_LAUNCH("kv8_dequantize");
    return LANTERN_OK;
}
