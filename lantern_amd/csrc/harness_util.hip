// harness_util.hip -- bookkeeping kernel of the synthetic benchmark harness (lantern_amd/harness.py), NOT part of
// the product API in include/lantern_hip.h: it appends one step's results to the device-side logs, feeds the bonus
// token back as the next step's sample token, wraps finished images and advances the device step counter, so that a
// whole verify step is a fixed sequence of kernels with fixed arguments (capturable once into a hipGraph per pool slot).
#include "common.h"

namespace lantern {
__global__ void harness_advance_kernel(int B, int n_lens, int ld, int64_t tokens_per_image, int64_t max_steps, int64_t step_host,
                                       int64_t *__restrict__ step_dev,
                                       const int32_t *__restrict__ st_best, const int32_t *__restrict__ st_alen,
                                       const int32_t *__restrict__ st_cnt, const int64_t *__restrict__ st_token,
                                       int32_t *__restrict__ log_best, int32_t *__restrict__ log_alen, int32_t *__restrict__ log_cnt,
                                       int64_t *__restrict__ log_token, int64_t *__restrict__ sample_token,
                                       int64_t *__restrict__ lens_next, const int64_t *__restrict__ lens_base,
                                       const double *__restrict__ u_bonus, double *__restrict__ u_cur) {
    const int64_t step = step_host >= 0 ? step_host : step_dev[0];   // eager launches know the step; graph replays read the device counter
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        if (step < max_steps) {
            log_best[step * ld + b] = st_best[b];
            log_alen[step * ld + b] = st_alen[b];
            log_token[step * ld + b] = st_token[b];
            for (int c = 0; c < 6; ++c) log_cnt[(step * ld + b) * 6 + c] = st_cnt[b * 6 + c];
        }
        sample_token[b] = st_token[b];
        if (step + 1 < max_steps) u_cur[b] = u_bonus[(step + 1) * ld + b];
    }
    for (int t = threadIdx.x; t < n_lens; t += blockDim.x)
        if (lens_next[t] - lens_base[t] >= tokens_per_image) lens_next[t] = lens_base[t];
    __syncthreads();
    if (threadIdx.x == 0) step_dev[0] = step + 1;
}
}  // namespace lantern

// B sequences of one group; `ld` = row stride (all sequences) of the step-major logs and of u_bonus
extern "C" int lantern_harness_advance(int B, int n_lens, int ld, int64_t tokens_per_image, int64_t max_steps, int64_t step_host,
                                       int64_t *step_dev,
                                       const int32_t *st_best, const int32_t *st_alen, const int32_t *st_cnt, const int64_t *st_token,
                                       int32_t *log_best, int32_t *log_alen, int32_t *log_cnt, int64_t *log_token, int64_t *sample_token,
                                       int64_t *lens_next, const int64_t *lens_base, const double *u_bonus, double *u_cur, void *stream) {
    hipLaunchKernelGGL(lantern::harness_advance_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, B, n_lens, ld, tokens_per_image, max_steps,
                       step_host, step_dev, st_best, st_alen, st_cnt, st_token, log_best, log_alen, log_cnt, log_token, sample_token, lens_next,
                       lens_base, u_bonus, u_cur);
    LANTERN_CHECK_LAUNCH("harness_advance");
    return LANTERN_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// Do two streams share a hardware queue?  (The runtime maps every stream to one of a few hardware queues when the stream is first used, and
// offers no way to ask which.)  A hardware queue runs its packets in order, so: a one-wave kernel on stream A polls a flag for at most
// PROBE_TICKS of the constant-rate wall clock (100 MHz: ~200 us) and records whether it saw it; a one-thread kernel enqueued right behind it on
// stream B sets the flag.  On distinct queues the second kernel runs beside the first, which sees the flag within microseconds; on one queue
// it waits behind the first, which times out.
namespace lantern {
constexpr long long PROBE_TICKS = 20000;

__global__ void queue_probe_wait_kernel(int *__restrict__ flag, int *__restrict__ saw) {
    if (threadIdx.x != 0) return;
    const long long t0 = wall_clock64();
    int seen = 0;
    for (int spins = 0; spins < 100000 && !seen; ++spins) {          // (the count only backstops a clock that does not advance)
        seen = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        if (wall_clock64() - t0 > PROBE_TICKS) break;
        __builtin_amdgcn_s_sleep(8);
    }
    saw[0] = seen;
}

__global__ void queue_probe_set_kernel(int *__restrict__ flag) { __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
}  // namespace lantern

// *shared = 1 if work on stream_b cannot start while a kernel on stream_a runs (one hardware queue; a stream against itself), else 0.  Synchronises both
// streams.  "Shared" only after three attempts in a row timed out: a host hiccup between the two launches of one attempt must not read as a shared queue.
extern "C" int lantern_streams_share_queue(void *stream_a, void *stream_b, int *shared) {
    if (!shared) {
        lantern::set_error("streams_share_queue: shared is NULL");
        return LANTERN_E_INVALID;
    }
    hipStream_t a = (hipStream_t)stream_a, b = (hipStream_t)stream_b;
    int *dev = nullptr;          // [0] the flag, [1] what the waiting kernel saw
    if (hipMalloc(&dev, 2 * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        lantern::set_error("streams_share_queue: hipMalloc failed");
        return LANTERN_E_LAUNCH;
    }
    int rc = LANTERN_OK, saw = 0;
    for (int attempt = 0; attempt < 3 && rc == LANTERN_OK && !saw; ++attempt) {
        // both streams idle and the flag cleared before either kernel is enqueued
        if (hipMemsetAsync(dev, 0, 2 * sizeof(int), a) != hipSuccess || hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) {
            rc = LANTERN_E_LAUNCH;
            break;
        }
        hipLaunchKernelGGL(lantern::queue_probe_wait_kernel, dim3(1), dim3(64), 0, a, dev, dev + 1);
        hipLaunchKernelGGL(lantern::queue_probe_set_kernel, dim3(1), dim3(1), 0, b, dev);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess ||
            hipMemcpy(&saw, dev + 1, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess)
            rc = LANTERN_E_LAUNCH;
    }
    (void)hipFree(dev);
    if (rc != LANTERN_OK) {
        (void)hipGetLastError();
        lantern::set_error("streams_share_queue: a launch, copy or synchronise failed");
        return rc;
    }
    *shared = saw ? 0 : 1;
    return LANTERN_OK;
}
