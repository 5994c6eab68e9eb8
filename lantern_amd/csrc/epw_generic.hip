// epw_generic.hip -- the argument-driven instances of the windowed chain kernel (epw_body.h, SPEC 0: mode, flags and sizes from the argument
// block; one workgroup per CU), by window width and neighbour-id mode; and the same with TopPLogitsWarper compiled in for rows that arrive as
// logits (LANTERN_ROWS_LOGITS with prm.top_p in (0, 1): drafters/utils.py:36-52 -- the reference applies the processor list per visited row
// inside evaluate_posterior, ea_model_llamagen.py:709-787).
#undef EPW_TRACE
#include "epw_body.h"

namespace lantern {

// threads x float4 per thread by window width (<= 1024, 2048, 4096, 8192, 16384 ids: epw_select's generic()), each for the three neighbour-id modes
#define EPW_GENERIC_IDS(NT, E4, TPO) \
    EPW_CHAIN(NT, E4, 2, 1, false, false, EPW_SPEC_GENERIC, TPO) EPW_CHAIN(NT, E4, 1, 1, false, false, EPW_SPEC_GENERIC, TPO) EPW_CHAIN(NT, E4, 0, 1, false, false, EPW_SPEC_GENERIC, TPO)
#define EPW_GENERIC_WIDTHS(TPO) \
    EPW_GENERIC_IDS(256, 1, TPO) EPW_GENERIC_IDS(256, 2, TPO) EPW_GENERIC_IDS(512, 2, TPO) EPW_GENERIC_IDS(512, 4, TPO) EPW_GENERIC_IDS(1024, 4, TPO)
EpwInstanceList epw_generic_instances() {
    static const EpwInstance k[] = {EPW_GENERIC_WIDTHS(EPW_NUCLEUS) EPW_GENERIC_WIDTHS(0)};
    return {k, (int)(sizeof(k) / sizeof(k[0]))};
}

}  // namespace lantern
