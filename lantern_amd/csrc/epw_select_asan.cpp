// epw_select_asan.cpp -- the chain kernel's instance selection under AddressSanitizer + UBSan, as a program of its own (`make asan-select`): it links the
// host-only sanitizer build of the library and walks lantern_evaluate_posterior_window_instance -- epw_check, epw_spec_matches, epw_select, epw_find and the
// name formatting -- over the product configurations and the tuning values that move the selection.  Nothing is launched and no device pointer is
// dereferenced, so the argument blocks carry a dummy pointer.  Exit status 0: every name as expected and no sanitizer report (a report ends the program).
#include <climits>
#include <cstdio>
#include <cstring>

#include "../../include/lantern_hip.h"

static int failures = 0;
static void *const PTR = (void *)0x1000;

struct Blocks {
    lantern_ep_params prm;
    lantern_ep_buffers buf;
    lantern_ep_window win;
};

// Lumina-mGPT (V 65536, image ids [4, 8196)) on a static tree or on per-sequence trees; LlamaGen otherwise (V 16384, LANTERN off, per-sequence trees)
static Blocks blocks(bool lumina, bool is_static, int B, int P, int D, int N, int rows_kind) {
    Blocks b;
    memset(&b, 0, sizeof(b));
    lantern_ep_params &p = b.prm;
    p.B = B, p.P = P, p.D = D, p.rows_per_seq = N, p.n_uniforms = 64, p.temperature = 1.0f, p.top_p = 1.0f, p.k = 1000, p.delta = 0.1;
    p.mode = is_static ? LANTERN_MODE_STATIC_LUMINA : LANTERN_MODE_DYNAMIC;
    p.R = is_static ? 1 : 0, p.N = is_static ? N : 0, p.row_index_per_seq = is_static ? 0 : 1;
    const bool raw = rows_kind == LANTERN_ROWS_RAW_BF16;
    if (lumina) {
        const int syntax[4] = {8196, 8197, 8803, 8828};
        p.V = 65536, p.tok_offset = 4, p.img_lo = 4, p.img_hi = 8196, p.syntax_shortcut = 1, p.n_syntax = 4, p.lantern = 1, p.table_rows = 8192, p.table_cols = 1024;
        memcpy(p.syntax, syntax, sizeof(syntax));
    } else {
        p.V = 16384, p.img_hi = raw ? 16384 : INT_MAX;          // raw rows: the window is the image-token range
    }
    lantern_ep_buffers &f = b.buf;
    f.logits = (const float *)PTR, f.row_index = (const int32_t *)PTR, f.cand = (const int64_t *)PTR, f.uniforms = (const double *)PTR;
    f.best = f.accept_len = f.counters = (int32_t *)PTR;
    if (is_static) {
        f.cart_prob = f.orig_prob = (const float *)PTR, f.op_off = f.p_idx = f.b_off = f.b_idx = (const int32_t *)PTR, f.tree_cand = (const int64_t *)PTR;
    } else {
        f.n_paths = f.n_depth = (const int32_t *)PTR;
    }
    if (lumina) f.nn_table = (const uint16_t *)PTR;
    lantern_ep_window &w = b.win;
    w.win_lo = p.img_lo, w.win_len = lumina ? 8192 : 16384, w.orig_prob_stride = w.win_len, w.rows_kind = rows_kind;
    if (raw) {
        w.raw_uncond = PTR, w.raw_probs = (const float *)PTR, w.raw_pre = (const uint8_t *)PTR, w.raw_pos_per_seq = is_static ? 0 : 1;
        if (lumina) {
            w.raw_pos_ids = w.raw_seq_len = (const int64_t *)PTR;
            w.raw_w_latent = w.raw_h_latent = 48, w.raw_newline_id = 8803, w.raw_eos_id = 8196;
        }
    }
    return b;
}

static void expect(const char *what, const Blocks &b, int fused, int want_rc, const char *want_name) {
    char name[96];
    const int rc = lantern_evaluate_posterior_window_instance(&b.prm, &b.buf, &b.win, fused, name, (int)sizeof(name));
    if (rc != want_rc || strcmp(name, want_name)) {
        fprintf(stderr, "%s: status %d name '%s' (%s), expected %d '%s'\n", what, rc, name, lantern_last_error(), want_rc, want_name);
        ++failures;
    }
}

int main() {
    const int PROBS = LANTERN_ROWS_PROBS, RAW = LANTERN_ROWS_RAW_BF16;
    lantern_tuning_reset();
    expect("lumina default tree 4096", blocks(true, true, 4096, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<256,8,2,4,true,false,2,205>");
    expect("lumina default tree 16", blocks(true, true, 16, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<512,4,2,1,true,false,2,0>");
    expect("lumina other tree 4096", blocks(true, true, 4096, 20, 5, 30, PROBS), 0, LANTERN_OK, "epw_kernel<256,8,2,3,true,false,1,9>");
    expect("lumina dynamic 4096", blocks(true, false, 4096, 20, 7, 60, PROBS), 0, LANTERN_OK, "epw_kernel<256,8,2,3,true,false,3,9>");
    expect("lumina raw 4096", blocks(true, true, 4096, 15, 6, 26, RAW), 0, LANTERN_OK, "epw_kernel<256,8,2,2,true,true,2,9>");
    expect("lumina raw fused 16", blocks(true, true, 16, 15, 6, 26, RAW), 1, LANTERN_OK, "epw_kernel_fused<512,4,2,1,true,true,2,0>");
    expect("lumina raw fused 257", blocks(true, true, 257, 15, 6, 26, RAW), 1, LANTERN_E_UNSUPPORTED, "");
    expect("llamagen 4096", blocks(false, false, 4096, 20, 7, 60, PROBS), 0, LANTERN_OK, "epw_kernel<512,8,1,4,true,false,5,777>");
    expect("llamagen 16", blocks(false, false, 16, 20, 7, 60, PROBS), 0, LANTERN_OK, "epw_kernel<1024,4,1,1,false,false,0,0>");
    expect("llamagen raw 16", blocks(false, false, 16, 20, 7, 60, RAW), 0, LANTERN_OK, "epw_kernel<1024,4,1,1,true,true,5,0>");
    Blocks lg = blocks(false, false, 16, 20, 7, 60, LANTERN_ROWS_LOGITS);
    lg.win.win_len = lg.win.orig_prob_stride = 2048, lg.prm.top_p = 0.9f;
    expect("logits top_p 2048", lg, 0, LANTERN_OK, "epw_kernel<256,2,1,1,false,false,0,2>");

    // the tuning values the selection reads
    lantern_tuning_set("epw_spec", 0);
    expect("epw_spec 0", blocks(true, true, 16, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<512,4,2,1,true,false,0,0>");
    lantern_tuning_reset();
    lantern_tuning_set("epw_occ2", 0);
    expect("epw_occ2 0", blocks(true, true, 4096, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<512,4,2,1,true,false,2,0>");
    lantern_tuning_reset();
    lantern_tuning_set("epw_tp4", 0);
    expect("epw_tp4 0", blocks(true, true, 4096, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<256,8,2,3,true,false,2,9>");
    lantern_tuning_set("epw_tp4", 3);
    expect("epw_tp4 3", blocks(true, true, 4096, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<256,8,2,4,true,false,2,85>");
    lantern_tuning_set("epw_tp", 1);
    expect("epw_tp 1", blocks(true, true, 4096, 15, 6, 26, PROBS), 0, LANTERN_OK, "epw_kernel<512,4,2,4,true,false,2,0>");
    lantern_tuning_reset();
    lantern_tuning_set("epw_tp_raw", 512);
    expect("epw_tp_raw 512", blocks(true, true, 4096, 15, 6, 26, RAW), 0, LANTERN_OK, "epw_kernel<512,4,2,4,true,true,2,1>");
    lantern_tuning_set("epw_tp_lg", 4);
    expect("epw_tp_lg 4", blocks(false, false, 4096, 20, 7, 60, PROBS), 0, LANTERN_OK, "epw_kernel<512,8,1,4,true,false,5,905>");
    lantern_tuning_reset();

    // the argument checks come first; a name needs room (the buffer's end is where ASan would see an overrun)
    Blocks bad = blocks(true, true, 16, 15, 6, 26, PROBS);
    bad.buf.cand = nullptr;
    expect("null cand", bad, 0, LANTERN_E_INVALID, "");
    const Blocks ok = blocks(true, true, 16, 15, 6, 26, PROBS);
    for (int cap = 1; cap <= 40; ++cap) {
        char *small = new char[cap];
        const int rc = lantern_evaluate_posterior_window_instance(&ok.prm, &ok.buf, &ok.win, 0, small, cap);
        const int want = cap > (int)strlen("epw_kernel<512,4,2,1,true,false,2,0>") ? LANTERN_OK : LANTERN_E_INVALID;
        if (rc != want) fprintf(stderr, "cap %d: status %d, expected %d\n", cap, rc, want), ++failures;
        delete[] small;
    }
    if (lantern_evaluate_posterior_window_instance(&ok.prm, &ok.buf, &ok.win, 0, nullptr, 0) != LANTERN_E_INVALID) ++failures;
    printf("epw_select_asan: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
