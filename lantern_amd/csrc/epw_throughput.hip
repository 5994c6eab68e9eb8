// epw_throughput.hip -- the forms of the windowed chain kernel (epw_body.h) for more sequences per launch than CUs: several workgroups share a
// CU, the register allocation is capped accordingly (WPE), the fixed configurations (SPEC) fold their flags away, and a candidate's drafter row is
// requested only once its rejection is known (EPW_LATE_Q).  BASELINE assesses evaluate_posterior's roofline target at this batch.
//   256 threads x 8 float4, three workgroups per CU (53 KB of LDS each): probability rows and -- round 5 -- raw cond / uncond bf16 rows
//   512 threads x 4 float4 at 128 VGPRs, two per CU: everything else on the 8192-id window
//   512 threads x 8 float4 at 128 VGPRs, two per CU (79 KB of LDS each): LlamaGen's 16384-id window, standard verify on dynamic trees (round 6)
// Which tuning value picks which of the measurement variants below: epw_select (window_kernels.hip).
#undef EPW_TRACE
#include "epw_body.h"

namespace lantern {

EpwInstanceList epw_throughput_instances() {
    static const EpwInstance k[] = {
        // The default tree on the smallest staged tables: 40 KB of LDS, 128 VGPRs -- FOUR workgroups per CU (below in the order epw_tp4 = 2, 3, 4, 1).  epw_tp4 = 1 (default, round 6): the serial wave
        // rotates with the sequence and runs at raised priority, a rejection's residual is normalised by a second pass over LDS (no spills): 135.9 - 137.8 us
        // per 4096 sequences against round 5's 147.8 - 157.5 on the same boxes; 2 = round 5's compact form; 3 = the neighbour scan on all waves instead of
        // the rotation (139.5 - 140.1); 4 = 1 without the raised priority (137.5 - 137.8); 0 = round 4's three-per-CU form (162 - 163)
        EPW_CHAIN(256, 8, 2, 4, true, false, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q | EPW_COMPACT)
        EPW_CHAIN(256, 8, 2, 4, true, false, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q | EPW_COMPACT | EPW_ALLW | EPW_LDS2P)
        EPW_CHAIN(256, 8, 2, 4, true, false, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q | EPW_COMPACT | EPW_ROTW | EPW_LDS2P)
        EPW_CHAIN(256, 8, 2, 4, true, false, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q | EPW_COMPACT | EPW_ROTW | EPW_LDS2P | EPW_PRIO)
        // the fixed configurations on probability rows: 256 threads x 8 float4, three per CU
        EPW_CHAIN(256, 8, 2, 3, true, false, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q | EPW_ROTW)
        EPW_CHAIN(256, 8, 2, 3, true, false, EPW_SPEC_LUMINA_STATIC, EPW_LATE_Q | EPW_ROTW)
        EPW_CHAIN(256, 8, 2, 3, true, false, EPW_SPEC_LUMINA_DYNAMIC, EPW_LATE_Q | EPW_ROTW)
        EPW_CHAIN(256, 8, 2, 3, true, false, EPW_SPEC_ANOLE_STATIC, EPW_LATE_Q | EPW_ROTW)
        // 512 threads at 128 VGPRs, two per CU: the older forms of the default tree and of the packed 8192-id window, then any table form
        EPW_CHAIN(512, 4, 2, 4, true, false, EPW_SPEC_LUMINA_DEFAULT_TREE, 0)
        EPW_CHAIN(512, 4, 2, 4, true, false, EPW_SPEC_GENERIC, 0)
        EPW_CHAIN(512, 4, 0, 4, false, false, EPW_SPEC_GENERIC, 0)
        EPW_CHAIN(512, 4, 1, 4, false, false, EPW_SPEC_GENERIC, 0)
        EPW_CHAIN(512, 4, 2, 4, false, false, EPW_SPEC_GENERIC, 0)
        // raw rows carry the row post-process's 18 KB of histograms: 71 KB of LDS per workgroup = two per CU whatever the thread count.  256 threads x 8
        // float4 at two waves per SIMD (no register cap to spill against, half the waves -- half the repeated scalar work -- per sequence), or
        // (epw_tp_raw = 512) 512 threads at 128 VGPRs
        EPW_CHAIN(512, 4, 2, 4, true, true, EPW_SPEC_GENERIC, 0)
        EPW_CHAIN(512, 4, 2, 4, true, true, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q)
        EPW_CHAIN(256, 8, 2, 2, true, true, EPW_SPEC_LUMINA_DEFAULT_TREE, EPW_LATE_Q | EPW_ROTW)
        EPW_CHAIN(512, 4, 2, 4, true, true, EPW_SPEC_LUMINA_STATIC, EPW_LATE_Q)
        EPW_CHAIN(256, 8, 2, 2, true, true, EPW_SPEC_LUMINA_STATIC, EPW_LATE_Q | EPW_ROTW)
        EPW_CHAIN(512, 4, 2, 4, true, true, EPW_SPEC_LUMINA_DYNAMIC, EPW_LATE_Q)
        EPW_CHAIN(256, 8, 2, 2, true, true, EPW_SPEC_LUMINA_DYNAMIC, EPW_LATE_Q | EPW_ROTW)
        EPW_CHAIN(512, 4, 2, 4, true, true, EPW_SPEC_ANOLE_STATIC, EPW_LATE_Q)
        EPW_CHAIN(256, 8, 2, 2, true, true, EPW_SPEC_ANOLE_STATIC, EPW_LATE_Q | EPW_ROTW)
        // LlamaGen's standard verify (BASELINE config 2) on probability rows: the 64 KB window + EwSharedLite + the per-path tables = <= 80 KB, TWO workgroups of
        // 512 threads x 8 float4 per CU at 128 VGPRs (the generic instance: 1024 threads, 97 KB, one per CU).  (below in the order epw_tp_lg = 2, 3, 4, 1).  epw_tp_lg = 1: rows by LDS-DMA; 2: rows through
        // registers + the residual normalised by a second LDS pass; 3: rows through registers; 4: 1 + raised priority of the serial section
        EPW_CHAIN(512, 8, 1, 4, true, false, EPW_SPEC_LLAMAGEN_DYNAMIC, EPW_LATE_Q | EPW_ROTW | EPW_LDS2P | EPW_LITE)
        EPW_CHAIN(512, 8, 1, 4, true, false, EPW_SPEC_LLAMAGEN_DYNAMIC, EPW_LATE_Q | EPW_ROTW | EPW_LITE)
        EPW_CHAIN(512, 8, 1, 4, true, false, EPW_SPEC_LLAMAGEN_DYNAMIC, EPW_LATE_Q | EPW_ROTW | EPW_PRIO | EPW_LITE | EPW_DMAROW)
        EPW_CHAIN(512, 8, 1, 4, true, false, EPW_SPEC_LLAMAGEN_DYNAMIC, EPW_LATE_Q | EPW_ROTW | EPW_LITE | EPW_DMAROW)
    };
    return {k, (int)(sizeof(k) / sizeof(k[0]))};
}

}  // namespace lantern
