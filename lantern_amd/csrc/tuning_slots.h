// tuning_slots.h -- the tuning values (lantern_tuning_set / lantern_tuning_get), listed ONCE: slot, name, default.  No HIP header: common.h takes the
// enum from here, tree_static.cpp the name / default table, so the two cannot fall out of step.
// Kernel-instance and launch-shape choices a measurement may want to override.  They are arguments of an explicit C-ABI call -- the library reads
// NO environment variable (round 5's getenv knobs are gone); the defaults below are what every product path runs.
#pragma once

#define LANTERN_TUNING_SLOTS(X)                                                                                                                                  \
    X(EPW_TP, "epw_tp", 5)                        /* throughput instances of the chain kernel for > 256 sequences per launch (0: generic two-per-CU instance; 1..4: older forms) */ \
    X(EPW_TP4, "epw_tp4", 1)                      /* the compact four-per-CU instance for the default tree; 0: round 4's three-per-CU form */                    \
    X(EPW_TP_RAW, "epw_tp_raw", 256)              /* threads per sequence of the raw-row throughput instances (512: the 128-VGPR form) */                        \
    X(EPW_SPEC, "epw_spec", 2)                    /* fixed-configuration instances (1: no fixed tree, 0: the generic instance) */                                \
    X(EPW_OCC2, "epw_occ2", -1)                   /* throughput forms when B > 256 (0 / 1 force them off / on) */                                                \
    X(O7_NT, "o7_nt", 0)                          /* threads per row of cfg_window_bf16_kernel by window size (256 / 1024 force a form) */                       \
    X(PREP_NT, "prep_nt", 0)                      /* prep_rows_kernel<512> (1024: the 1024-thread form) */                                                       \
    X(KV_U, "kv_u", 0)                            /* 0 -> 2 row groups in flight per thread of the KV mover */                                                   \
    X(KV_KS, "kv_ks", 4)                          /* slabs per workgroup of the small-slab commit kernel (0: one workgroup tile per slab) */                     \
    X(KV_VARIANT, "kv_variant", 0)                /* 10 * U + mode of the KV mover (measurement variants) */                                                     \
    X(GEMM_TILED_FROM, "gemm_tiled_from", 129)    /* rows from which lantern_linear_rows_packed runs the LDS-tiled GEMM */                                       \
    X(SK_GROUPS, "sk_groups", 0)                  /* stream-K grid = one workgroup per CU (> 0 forces the grid) */                                               \
    X(SK_WHOLE_MB, "sk_whole_mb", 40)             /* matrices up to this many MB get whole tiles per workgroup */                                                \
    X(SK_NT_MIN_MB, "sk_nt_min_mb", 80)           /* matrices from this many MB are streamed with non-temporal loads */                                          \
    X(TA_SPLITS, "ta_splits", 0)                  /* key splits of tree attention by launch size (> 0 forces the split count) */                                 \
    X(TA_MIN_TILES, "ta_min_tiles", 2)            /* key tiles per wave and split below which no further split is made */                                        \
    X(EPW_TP_LG, "epw_tp_lg", 1)                  /* LlamaGen's 16384-id throughput instance (two per CU, rows by LDS-DMA); 2: + second LDS pass for the residual; 3: rows through registers; 4: + raised priority; 0: off */ \
    X(EPW_FUSED_HELPERS, "epw_fused_helpers", 1)  /* helper workgroups per sequence of the chain launch that carries its prepare stage (LANTERN_STEP_FUSED_PREPARE) */

namespace lantern {
enum Tuning {
#define LANTERN_TUNING_ENUM(id, name, dflt) TUNE_##id,
    LANTERN_TUNING_SLOTS(LANTERN_TUNING_ENUM)
#undef LANTERN_TUNING_ENUM
    TUNE_COUNT
};
}  // namespace lantern
