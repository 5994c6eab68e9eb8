"""The batch-of-one verify step of the mirror classes through ONE lantern_verify_step call.

`OneCallStep` is the one place that knows how a lantern_step_group for such a step is built, launched and read back: the C structs,
the preallocated buffers and the word layout of the verdict record.  It knows nothing about a model family -- every difference between
the mirrors (grammar, window, processors, tree kind, O8 form, where the verdict is read, which length tensors the commit advances)
arrives as a constructor argument or as a per-step value.  What stays with the mirrors: the target forwards, the uniforms, the dense
retry, `input_ids` and the drafter call.

A step is: begin() -> gather_candidates() | bind_tree() -> bind_rows() / bind_orig_prob() / bind_hidden*() / bind_bonus() /
bind_lengths() / bind_ids() -> launch() -> verdict() -> end().  From begin() to the next begin(), `token` (the bonus token, [1] i64)
and `out_hidden` ([1, 2, D, H]) are this step's.  `parity` (0 / 1) names the record the running step writes: begin() does not change it, only
end() flips it, so a mirror that double-buffers tensors of its own (KV lengths) indexes them with `parity` between begin() and end().
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib, ops
from .verify import concat_original_prob

MAX_DEPTH, MAX_ROWS = 8, 64          # what one group takes: paths of at most 8 tokens, a static tree of at most 64 rows


def slabs_alike(slabs) -> bool:
    """One commit launch moves every slab: same shape, dtype and device, all contiguous."""
    s0 = slabs[0]
    return all(x.shape == s0.shape and x.dtype == s0.dtype and x.device == s0.device and x.is_contiguous() for x in slabs)


def row_index_of(retrieve: torch.Tensor, N: int) -> torch.Tensor:
    """retrieve [P, D] i64 (-1 behind a path's end) -> the rows evaluate_posterior reads, i32 (no host read: EAGLE-2 steps call this)."""
    return torch.where(retrieve < 0, retrieve + N, retrieve).to(torch.int32).contiguous()


class OneCallStep:
    def __init__(self, slabs, slab_ptrs, slab_seq, *, N, P, D, R, V, win_lo, win_len, ep_cfg: ops.EpConfig, model, cfg_scale, top_k,
                 temperature=1.0, top_p=1.0, img_lo=0, img_hi=0, pos_ids=None, pos_base=0, w_latent=0, h_latent=0, newline_id=0, eos_id=0, fifo=None, table=None,
                 tree=None, nodes=None, greedy=None, pinned_verdict=False, ids=None, ids_cap=0):
        """`tree`: the static tree's tables (tree_indices, retrieve, op_off, p_idx, b_off, b_idx) -- None: every step brings its own tree
        (bind_tree).  `w_latent / h_latent / newline_id / eos_id`: the grid of a position-dependent O7 mask.  `fifo`: the acceptance uniforms
        (None: nothing is drawn).  `nodes`: ops.NodeTables -> the node-parallel O8.  `greedy`: dict(lantern, k, delta, tok_offset, table) ->
        the greedy / TVD accept as the O8 stage (the record's counter words then stay zero).  `pinned_verdict`: evaluate_posterior also writes
        the record to pinned host memory and verdict() polls it there.  `ids`: [1, L] ids the commit appends to in place, in a buffer of
        `ids_cap` columns."""
        s0 = slabs[0]
        dev = self.dev = s0.device
        self.L, self.N, self.P, self.D = _lib.lib(), N, P, D
        z = lambda *shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        self.cand, self.cart, self.tcand = z(1, max(P, 1), max(D, 1), dt=torch.int64), z(1, max(P, 1), max(D, 1), dt=torch.float32), z(1, N, dt=torch.int64)
        self.win, self.hot = z(N, win_len, dt=torch.float32), z(N, dt=torch.int32)
        # the verdict record, double-buffered (the drafter keeps the previous step's bonus token / hidden rows while this step's are written):
        # best, accept_len, counters[6], bonus token (int64 at words 8-9)
        self.recs = [z(16, dt=torch.int32), z(16, dt=torch.int32)]
        self.toks = [r[8:10].view(torch.int64) for r in self.recs]
        self._rec_ptrs = [(r.data_ptr(), t.data_ptr()) for r, t in zip(self.recs, self.toks)]          # (host time: data_ptr() once, not per step)
        self.otok, self.omass = z(1, dt=torch.int32), z(1, dt=torch.float32)
        self.acc = z(1, MAX_DEPTH, dt=torch.int64)
        # the accepted hidden rows stay per parity: the drafter reads the previous step's rows while this step's are written
        self._out_flat, self._out_views = [None, None], [None, None]
        self.rec = self.token = self.out_hidden = None
        self.parity = 0
        # what a step's bind_*() converted or built: alive until the launch has been queued.  Dropping them there is safe because the launch and
        # every later torch allocation run on ONE stream (`a.stream`, captured below): the caching allocator reuses a freed block only behind
        # the kernels already queued on it.  A step driven from a second stream would have to keep them until the verdict is read.
        self._live = []
        self.group = (_lib.StepGroup * 1)()
        a = self.a = self.group[0]
        p, b, w = a.ep, a.ep_buf, a.ep_win
        self.eb, self.ew = b, w
        a.stream = torch.cuda.current_stream().cuda_stream          # (generate() runs on one stream)
        # ss_token NULL + CANDIDATES_READY: lantern_verify_step takes the candidates as gather_candidates() / bind_tree() leave them -- no second O6 launch
        a.ss_token, a.flags = None, _lib.STEP_CANDIDATES_READY
        a.B, a.N, a.P, a.D = 1, N, P, D
        a.tree_cand, a.cand, a.cart_prob = self.tcand.data_ptr(), self.cand.data_ptr(), self.cart.data_ptr()
        # ---- O7: CFG + the model's mask + the processors, every row a window of probabilities
        self.pos_ids = pos_ids
        a.V, a.cfg, a.model, a.img_lo, a.img_hi = V, float(cfg_scale), model, img_lo, img_hi
        a.pos_ids, a.pos_base = (pos_ids.data_ptr() if pos_ids is not None else None), pos_base
        a.w_latent, a.h_latent, a.newline_id, a.eos_id = w_latent, h_latent, newline_id, eos_id
        a.top_k, a.win_lo, a.win_len, a.out_kind = top_k, win_lo, win_len, ops.ROWS_PROBS
        a.out_win, a.row_hot, a.temperature, a.top_p = self.win.data_ptr(), self.hot.data_ptr(), float(temperature), float(top_p)
        # ---- O8: the rows are final probabilities (the processors ran in the O7 stage)
        self.table = table
        ops.fill_ep_params(p, ep_cfg, B=1, P=P, D=D, V=V, rows_per_seq=N, n_uniforms=0 if fifo is None else fifo.buf.shape[1],
                           top_k=0, temperature=1.0, top_p=1.0, R=R, N=N, table_shape=None if table is None else table.shape)
        b.logits, b.nn_table = self.win.data_ptr(), (table.data_ptr() if table is not None else None)
        self.tree = tree
        if tree is not None:
            self.tree_indices, self.retrieve = tree["tree_indices"].to(dev).contiguous(), tree["retrieve"].to(dev).contiguous()
            self.row_index = row_index_of(self.retrieve, N)
            a.tree_indices, a.retrieve = self.tree_indices.data_ptr(), self.retrieve.data_ptr()
            b.row_index, b.cand, b.cart_prob, b.tree_cand = self.row_index.data_ptr(), a.cand, a.cart_prob, a.tree_cand
            b.op_off, b.p_idx, b.b_off, b.b_idx = (tree[k].data_ptr() for k in ("op_off", "p_idx", "b_off", "b_idx"))
        if fifo is not None:
            b.uniforms, b.cursor = fifo.buf.data_ptr(), fifo.cursor.data_ptr()
        w.win_lo, w.win_len, w.row_hot, w.rows_kind = win_lo, win_len, self.hot.data_ptr(), ops.ROWS_PROBS
        w.orig_prob_stride, w.orig_prob_offset = V, win_lo
        w.out_tok, w.out_mass = self.otok.data_ptr(), self.omass.data_ptr()
        if nodes is not None:
            nbytes = int(self.L.lantern_evaluate_posterior_nodes_workspace(C.byref(p), C.byref(w), nodes.n_internal, 0))
            self.nodes_ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            self.nodes_struct = nodes.struct(self.nodes_ws.data_ptr(), nbytes, -1)
            a.nodes = C.pointer(self.nodes_struct)
        self.gq = None
        if greedy is not None:
            # the dense f32 rows of the O7 stage, the accepted row, the scratch of the (path, depth) cells (sized for any tree the group takes)
            self.g_logits, self.g_out, self.g_ok = z(max(N, MAX_ROWS), V, dt=torch.float32), z(1, V, dt=torch.float32), z(MAX_ROWS * MAX_DEPTH, dt=torch.int32)
            self.g_table = greedy["table"]
            q = self.gq = _lib.StepGreedy()
            q.logits, q.out_row, q.ok_scratch = self.g_logits.data_ptr(), self.g_out.data_ptr(), self.g_ok.data_ptr()
            q.lantern, q.k, q.delta, q.tok_offset = int(bool(greedy["lantern"])), int(greedy["k"]), float(greedy["delta"]), int(greedy["tok_offset"])
            if self.g_table is not None:
                q.nn_table = self.g_table.data_ptr()
                q.table_rows, q.table_cols = self.g_table.shape
            q.win_lo, q.win_len = win_lo, win_len
            if tree is not None:
                q.row_index = self.row_index.data_ptr()
            a.greedy = C.pointer(q)
            a.out_win, a.top_k = None, 0
        # (host time: the constant arguments of lantern_gather_candidates as ctypes objects, once; greedy decoding has no candidate probabilities)
        self._gc_const = tuple(C.c_void_p(x) for x in (a.tree_indices, a.retrieve, a.tree_cand, a.cand, None if greedy is not None else a.cart_prob, a.stream))
        # ---- O9 + O10: every slab in one launch
        self.slab_ptrs, self.slab_seq = slab_ptrs, slab_seq
        a.slab_ptrs, a.slab_seq = slab_ptrs.data_ptr(), slab_seq.data_ptr()
        S, d = s0.shape[-2], s0.shape[-1]
        a.n_slabs, a.elem_bytes, a.outer, a.S_max, a.d = len(slabs), s0.element_size(), s0.numel() // (S * d), S, d
        a.accepted_tokens, a.hid_groups = self.acc.data_ptr(), 2
        self.verdict_np = None
        if pinned_verdict:
            try:
                self.verdict_pinned = torch.zeros(16, dtype=torch.int32).pin_memory()
                self.verdict_np = self.verdict_pinned.numpy()
                w.verdict_host = self.verdict_pinned.data_ptr()
            except RuntimeError:
                self.verdict_np = None
        self.ids_buf = None
        if ids is not None:
            self.ids_buf = torch.zeros((1, ids_cap), dtype=torch.int64, device=dev)
            self.ids_buf[:, :ids.shape[1]] = ids
            a.ids_buf, a.ids_stride = self.ids_buf.data_ptr(), ids_cap

    # ------------------------------------------------------------------ one step
    def begin(self):
        """This parity's record takes the step's verdict."""
        par = self.parity
        self.rec, self.token, self.out_hidden = self.recs[par], self.toks[par], None
        rp, tp = self._rec_ptrs[par]
        eb = self.eb
        eb.best, eb.accept_len, self.ew.token = rp, rp + 4, tp
        if self.gq is None:
            eb.counters = rp + 8
        else:          # no uniforms, no counters: the record's counter words stay zero
            eb.counters, self.gq.token = None, tp

    def gather_candidates(self, ss_token, ss_prob, sample_token):
        """O6 for the static tree, its own call because the target forward needs the tree tokens: fills `tcand`, `cand`, `cart`.
        (Host time is what a batch-of-one step costs: no-op conversions are skipped.)"""
        dev = self.dev
        if not (ss_token.device == dev and ss_token.is_contiguous()):
            ss_token = ss_token.to(dev).contiguous()
        if ss_prob is not None and not (ss_prob.device == dev and ss_prob.dtype == torch.float32 and ss_prob.is_contiguous()):
            ss_prob = ss_prob.to(dev).float().contiguous()
        if sample_token.device == dev and sample_token.is_contiguous():
            sample_token = sample_token.reshape(-1)
        else:
            sample_token = sample_token.to(dev).reshape(-1)[:1].contiguous()
        g = self._gc_const
        ops.check(self.L.lantern_gather_candidates(C.c_void_p(ss_token.data_ptr()), C.c_void_p(ss_prob.data_ptr() if ss_prob is not None else None),
                                                   C.c_void_p(sample_token.data_ptr()), g[0], g[1], 1, ss_token.numel(), self.N, self.P, self.D,
                                                   g[2], g[3], g[4], g[5]), "gather_candidates")

    def bind_tree(self, retrieve, cand, N) -> bool:
        """This step's EAGLE-2 tree: `retrieve` [P, D] i64 and `cand` [P, D] i64 (-1 behind a path's end) over N rows; P and D change from step
        to step and the group's fields follow them.  False: a tree outside what the group holds -- nothing was bound."""
        P, D = retrieve.shape
        if D > MAX_DEPTH or P < 1 or N < 1:
            return False
        a, eb = self.a, self.eb
        if self.gq is not None:
            if N > self.g_logits.shape[0] or P * max(D - 1, 1) > self.g_ok.numel():
                return False
        elif N > self.win.shape[0]:          # (a drafter whose trees grow: the row buffers follow)
            self.win = torch.zeros((N, self.win.shape[1]), dtype=torch.float32, device=self.dev)
            self.hot = torch.zeros(N, dtype=torch.int32, device=self.dev)
            a.out_win, a.row_hot, eb.logits, self.ew.row_hot = self.win.data_ptr(), self.hot.data_ptr(), self.win.data_ptr(), self.hot.data_ptr()
        row_index = row_index_of(retrieve, N)
        self.N, self.P, self.D = N, P, D
        a.N, a.P, a.D = N, P, D
        a.ep.rows_per_seq, a.ep.N, a.ep.P, a.ep.D = N, N, P, D
        a.retrieve, a.cand = retrieve.data_ptr(), cand.data_ptr()
        eb.row_index, eb.cand = row_index.data_ptr(), cand.data_ptr()
        if self.gq is not None:
            self.gq.row_index = row_index.data_ptr()
        self._live += (retrieve, cand, row_index)
        return True

    def bind_rows(self, cond, uncond):
        """The target's [N, V] logit rows of the two passes, bf16 or f32 alike (anything else goes through f32).  Returns them as bound."""
        if cond.dtype != uncond.dtype or cond.dtype not in (torch.bfloat16, torch.float32):
            cond, uncond = cond.float(), uncond.float()
        if not cond.is_contiguous():
            cond = cond.contiguous()
        if not uncond.is_contiguous():
            uncond = uncond.contiguous()
        a = self.a
        a.cond, a.uncond, a.dtype = cond.data_ptr(), uncond.data_ptr(), int(cond.dtype == torch.bfloat16)
        self._live += (cond, uncond)
        return cond, uncond

    def bind_orig_prob(self, levels):
        """The drafter's distributions, level by level, as one [R, V] f32 block (no copy when the levels already sit back to back)."""
        first = end = levels[0].data_ptr()
        for o in levels:
            if o.data_ptr() != end or o.dtype != torch.float32 or o.device != self.dev or not o.is_contiguous():
                orig = concat_original_prob(levels)
                first = orig.data_ptr()
                break
            end += 4 * o.numel()
        else:
            orig = levels
        self.eb.orig_prob = first
        self._live.append(orig)

    def bind_hidden(self, hidden):
        """The two passes' hidden rows stacked, [1, 2, N, H].  Returns this step's accepted-hidden output [1, 2, D, H]."""
        hidden = hidden.contiguous()
        self.a.hidden, self.a.hidden_uncond = hidden.data_ptr(), None
        self._live.append(hidden)
        return self._bind_out_hidden(hidden)

    def bind_hidden_pair(self, h0, h1):
        """The two passes' [N, H] hidden rows as two pointers when they are alike -- nothing is stacked -- else as bind_hidden()."""
        dev = self.dev
        if not (h0.is_contiguous() and h1.is_contiguous() and h0.dtype == h1.dtype and h0.shape == h1.shape and h0.device == dev and h1.device == dev):
            return self.bind_hidden(torch.stack((h0, h1))[None])
        self.a.hidden, self.a.hidden_uncond = h0.data_ptr(), h1.data_ptr()
        self._live += (h0, h1)
        return self._bind_out_hidden(h0)

    def _bind_out_hidden(self, like):
        par, D, H = self.parity, self.D, like.shape[-1]
        out = self._out_views[par]
        if out is None or out.dtype != like.dtype or out.shape[-1] != H or out.shape[2] != D:
            flat = self._out_flat[par]
            if flat is None or flat.dtype != like.dtype or flat.numel() != 2 * MAX_DEPTH * H:
                flat = self._out_flat[par] = torch.zeros(2 * MAX_DEPTH * H, dtype=like.dtype, device=self.dev)
            out = self._out_views[par] = flat[:2 * D * H].view(1, 2, D, H)          # (the kernel's [B, G, D, H] layout for THIS step's depth)
        a = self.a
        a.out_hidden, a.hid_elem_bytes, a.H = out.data_ptr(), like.element_size(), H
        self.out_hidden = out
        return out

    def bind_bonus(self, u):
        """`u` [1] f64 on the device: the uniform of the bonus draw."""
        self.ew.u_bonus = u.data_ptr()
        self._live.append(u)

    def bind_lengths(self, slab_prev, new_len, seq_len=None):
        """[n_slabs] i64: every slab's length before the step, and where the commit writes the lengths after it; `seq_len` [1] i64 for a
        position-dependent O7 mask."""
        a = self.a
        a.slab_prev, a.new_len = slab_prev.data_ptr(), new_len.data_ptr()
        if seq_len is not None:
            a.seq_len = seq_len.data_ptr()

    def bind_ids(self, n_ids, ids_len) -> bool:
        """The commit appends the accepted tokens and, behind them, the bonus token to `ids_buf` at *ids_len when the buffer has room behind
        `n_ids` ids.  Returns whether it will."""
        inplace = self.ids_buf is not None and n_ids + self.D + 2 <= self.ids_buf.shape[1]
        self.a.ids_buf, self.a.ids_len = (self.ids_buf.data_ptr() if inplace else None), (ids_len.data_ptr() if inplace else None)
        return inplace

    def resync_ids(self, input_ids):
        """After a step that was committed outside the call: keep the in-place copy of input_ids in step."""
        if self.ids_buf is not None and input_ids.shape[1] <= self.ids_buf.shape[1]:
            self.ids_buf[:, :input_ids.shape[1]] = input_ids[:1]

    def launch(self):
        if self.verdict_np is not None:
            self.verdict_np[10] = 0
        ops.check(self.L.lantern_verify_step(self.group, 1), "verify_step")
        self._live.clear()

    def verdict(self):
        """The step's one host read -> (best, accept_len, n_used uniforms, status, bonus token).  With a pinned record: polled where
        evaluate_posterior wrote it (visible as soon as the walk is done, while the commit still runs) -- no copy, no stream synchronisation."""
        r = None
        vh = self.verdict_np
        if vh is not None:
            spins = 0
            while vh[10] == 0:
                spins += 1
                if spins > 2_000_000:          # (seconds: something is badly wrong -- take the synchronising read)
                    break
            if vh[10] != 0:
                r = vh[:10].tolist()
                r[8] = (r[8] & 0xffffffff) | (r[9] << 32)
        if r is None:
            r = self.rec.tolist()
        return r[0], r[1], r[5], r[7], r[8]

    def raise_on_status(self):
        ops.raise_on_status(self.rec[2:8].reshape(1, 6))

    def end(self):
        """The next step writes the other record / hidden rows."""
        self.parity ^= 1
