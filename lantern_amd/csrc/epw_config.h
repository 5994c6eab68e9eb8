// epw_config.h -- the fixed configurations of the windowed evaluate_posterior kernels, stated ONCE: the kernels (epw_body in epw_body.h, epn_node in
// node_kernels.hip) fold these constants in at compile time, and the host takes an instance built for a configuration only when epw_spec_matches()
// says the argument block is exactly that configuration -- both read the same record, so they cannot disagree.
// Plain constexpr C++: no HIP runtime, usable from device code and from host code alike.
#pragma once
#include "../../include/lantern_hip.h"

namespace lantern {

// SPEC template argument of epw_kernel / epw_kernel_fused / epn_kernel (an int there: the mangled kernel names carry the number)
enum EpwSpecId : int {
    EPW_SPEC_GENERIC = 0,               // everything from the argument block
    EPW_SPEC_LUMINA_STATIC = 1,         // Lumina-mGPT, one static tree for all sequences
    EPW_SPEC_LUMINA_DEFAULT_TREE = 2,   // = 1 on the sizes of the reference's default tree mc_sim_7b_63 (run.sh / generate_images.py)
    EPW_SPEC_LUMINA_DYNAMIC = 3,        // Lumina-mGPT, per-sequence EAGLE-2 trees
    EPW_SPEC_ANOLE_STATIC = 4,          // Anole, one static tree (LANTERN_MODE_STATIC_LG: the neighbour set zeroes q)
    EPW_SPEC_LLAMAGEN_DYNAMIC = 5,      // LlamaGen, per-sequence EAGLE-2 trees, standard verify (BASELINE config 2)
    EPW_SPEC_COUNT
};

// TPO template argument of the chain kernel: a set of these bits (what each one does is described where epw_body decodes it)
enum EpwOption : int {
    EPW_LATE_Q = 1,      // a candidate's drafter row is requested once its rejection is known
    EPW_NUCLEUS = 2,     // TopPLogitsWarper (prm.top_p) compiled in
    EPW_COMPACT = 4,     // the default tree on the smallest staged tables (EwSharedCompact), rows by LDS-DMA
    EPW_ROTW = 8,        // the serial section's wave rotates with the sequence
    EPW_ALLW = 16,       // the neighbour scan on all waves
    EPW_LDS2P = 64,      // a rejection's residual is normalised by a second pass over LDS
    EPW_PRIO = 128,      // the serial section runs at raised wave priority
    EPW_LITE = 256,      // LlamaGen's small staged tables (EwSharedLite)
    EPW_DMAROW = 512,    // probability rows land in LDS by LDS-DMA
    EPW_FUSED = 1024     // the prepare stage rides in the launch (set by epw_kernel_fused, never at a launch site)
};

// What an instance built for a SPEC assumes about its argument block.
struct EpwSpec {
    int V, win_lo, win_len;             // vocabulary and the window of ids a row holds
    int tok_offset, table_rows;         // neighbour table: row = token - tok_offset (0 rows: LANTERN off, no table)
    int img_lo, img_hi;                 // image-token range
    int mode;                           // LANTERN_MODE_*
    bool lantern, syntax_shortcut;
    int syntax[4];                      // the shortcut's syntax ids (n_syntax = 4)
    bool grammar;                       // raw rows: rows at a line's / the image's end are forced one-hot rows (Lumina's MultiModalLogitsProcessor)
    int eos_id, newline_id;             // ... on these ids (-1: the vocabulary has none).  Not the same fact as `grammar`: Anole has the Chameleon ids, and its
                                        // instances keep the code that writes them, but Anole's processors force no such rows, so the host gives an
                                        // argument block with grammar rows (raw_w_latent > 0) an Anole instance never
    int P, D, N, rows_per_seq;          // a fixed tree's sizes (0: from the argument block)
    int fan_out;                        // a fixed tree's largest number of children under a node
};

constexpr EpwSpec epw_chameleon_spec(int mode, bool syntax_shortcut, bool grammar, bool default_tree) {
    // the Chameleon vocabulary of Lumina-mGPT and Anole: 65536 ids, the 8192 image ids [4, 8196) are the window and the neighbour table's rows
    return EpwSpec{65536, 4, 8192, 4, 8192, 4, 8196, mode, true, syntax_shortcut, {8196, 8197, 8803, 8828}, grammar, 8196, 8803,
                   default_tree ? 15 : 0, default_tree ? 6 : 0, default_tree ? 26 : 0, default_tree ? 26 : 0, default_tree ? 4 : 0};
}
constexpr EpwSpec kEpwSpec[EPW_SPEC_COUNT] = {
    EpwSpec{},                                                                    // EPW_SPEC_GENERIC: nothing assumed (the kernels read no field of it)
    epw_chameleon_spec(LANTERN_MODE_STATIC_LUMINA, true, true, false),
    epw_chameleon_spec(LANTERN_MODE_STATIC_LUMINA, true, true, true),
    epw_chameleon_spec(LANTERN_MODE_DYNAMIC, true, true, false),
    epw_chameleon_spec(LANTERN_MODE_STATIC_LG, false, false, false),
    // LlamaGen: 16384 ids, all of them image ids and the window; LANTERN off, no syntax shortcut, no grammar rows
    EpwSpec{16384, 0, 16384, 0, 0, 0, 16384, LANTERN_MODE_DYNAMIC, false, false, {0, 0, 0, 0}, false, -1, -1, 0, 0, 0, 0, 0},
};

// epw_body turns a neighbour id into a window index with `id & (win_len - 1)` where the table's rows are the window: that needs a power of two
constexpr bool epw_table_windows_are_powers_of_two() {
    for (const EpwSpec &c : kEpwSpec)
        if (c.lantern && c.table_rows == c.win_len && (c.win_len & (c.win_len - 1)) != 0) return false;
    return true;
}
static_assert(epw_table_windows_are_powers_of_two(), "a fixed configuration whose neighbour table spans the window: win_len must be a power of two");

// Does the argument block say exactly what the instances of `spec` assume?  Everything epw_body / epn_node fold from the record is tested here;
// what only ONE launch site requires (which pointers are present, row kinds, staging limits, tuning values) stays at that site.
inline bool epw_spec_matches(int spec, const lantern_ep_params &p, const lantern_ep_window &w) {
    if (spec <= EPW_SPEC_GENERIC || spec >= EPW_SPEC_COUNT) return false;
    const EpwSpec &c = kEpwSpec[spec];
    // An upper end of the image range at or beyond the vocabulary excludes no token, so any such img_hi is the record's img_hi == V (LlamaGen's
    // callers pass INT_MAX with probability rows; with raw rows epw_check has already required img_hi == win_lo + win_len).
    const bool img_hi = p.img_hi == c.img_hi || (c.img_hi == c.V && p.img_hi >= c.V);
    if (!(p.V == c.V && w.win_lo == c.win_lo && w.win_len == c.win_len && p.tok_offset == c.tok_offset && p.img_lo == c.img_lo && img_hi)) return false;
    if ((p.lantern != 0) != c.lantern || (c.lantern && p.table_rows != c.table_rows) || p.mode != c.mode) return false;
    if ((p.syntax_shortcut != 0) != c.syntax_shortcut) return false;
    if (c.syntax_shortcut && !(p.n_syntax == 4 && p.syntax[0] == c.syntax[0] && p.syntax[1] == c.syntax[1] && p.syntax[2] == c.syntax[2] && p.syntax[3] == c.syntax[3]))
        return false;
    // raw rows take their class from the position when raw_w_latent > 0: the instance then writes the record's ids
    if (w.rows_kind == LANTERN_ROWS_RAW_BF16 && w.raw_w_latent != 0 && !(c.grammar && w.raw_eos_id == c.eos_id && w.raw_newline_id == c.newline_id)) return false;
    if (c.P && !(p.P == c.P && p.D == c.D && p.N == c.N && p.rows_per_seq == c.rows_per_seq)) return false;
    return true;
}

}  // namespace lantern
