"""How far an fp8 (e4m3fn, per-row scale) drafter moves from the bf16 drafter, on the committed drafter fixtures:
  * tests/golden/layer.npz, layer_lg.npz: every fixture layer that fits the HIP path (head_dim 64 / 128, sizes % 64 == 0) on its recorded inputs
    (a 2 x 9 call, then a 2 x 5 call behind its cache), the fixture's own weights;
  * tests/golden/lumina_drafter.npz, anole_drafter.npz: the recorded call sequence of a drafting loop (ids, positions, masks, tree blocks, cache lengths)
    replayed through a seeded drafters.cnets.Model (hidden 256, the HIP layer of the model family) in both formats.
Behind each, a seeded head over the image-token window; per row: how many of the bf16 drafter's 10 likeliest tokens are among the fp8 drafter's 10
(what the EAGLE-2 expansion keeps per node), and KL(p_bf16 || p_fp8) of the head distributions.  The weights are the fixtures' random ones
(N(0, 1/K)): what a trained checkpoint loses in accept length is not measurable without one.
usage: drafter_fp8_agreement.py [out.json]"""
import json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np
import torch
from lantern_amd.drafters import cnets

dev, bf = torch.device("cuda"), torch.bfloat16
WINDOW = 8192


def head_metrics(h16, h8, head):
    """rows [R, H] of both drafters -> (mean / min top-10 overlap, mean / max KL) of softmax(head(row)) over the window"""
    with torch.no_grad():
        p16 = torch.log_softmax(torch.nn.functional.linear(h16, head).float(), dim=-1)
        p8 = torch.log_softmax(torch.nn.functional.linear(h8, head).float(), dim=-1)
    t16, t8 = p16.topk(10, dim=-1).indices, p8.topk(10, dim=-1).indices
    overlap = (t16[:, :, None] == t8[:, None, :]).any(-1).float().sum(-1)
    kl = (p16.exp() * (p16 - p8)).sum(-1)
    top1 = (t16[:, 0] == t8[:, 0]).float().mean()
    return dict(rows=int(h16.shape[0]), top10_overlap_mean=round(float(overlap.mean()), 3), top10_overlap_min=int(overlap.min()), top1_agree=round(float(top1), 3),
                kl_mean=round(float(kl.mean()), 5), kl_max=round(float(kl.max()), 5),
                hidden_rel_diff=round(float((h16.float() - h8.float()).abs().max() / h16.float().abs().max()), 4))


def seeded_head(H, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(WINDOW, H, generator=g) / H ** 0.5 * 4.0).to(bf).to(dev)          # logits of a few units


def layer_fixtures():
    import test_drafter_layer as TL
    out = []
    for name in TL.CASES + TL.LG_CASES + TL.AN_CASES:
        lg, an = name.startswith("lg_"), name.startswith("an_")
        builder, gg = (TL.build_lg, TL.gl) if lg else ((TL.build_an, TL.gl) if an else (TL.build, TL.g))
        layers = [builder(name, dev, bf) for _ in range(2)]
        at, mlp = layers[0].self_attn, layers[0].mlp
        if at.head_dim not in (64, 128) or at.hidden_size % 64 or mlp.gate_proj.out_features % 64:
            continue
        layers[1].weight_format = "fp8"
        ys = []
        for layer in layers:
            kw0 = dict(freqs_cis=gg(name, "f0", dev)) if lg else {}
            kw1 = dict(freqs_cis=gg(name, "f1", dev)) if lg else {}
            with torch.no_grad():
                y0, kv0 = layer(gg(name, "x0", dev, bf), attention_mask=gg(name, "m0", dev), position_ids=gg(name, "pos0", dev), use_cache=True, **kw0)
                y1, _ = layer(gg(name, "x1", dev, bf), attention_mask=gg(name, "m1", dev), position_ids=gg(name, "pos1", dev), past_key_value=kv0, use_cache=True, **kw1)
            ys.append(torch.cat([y0.reshape(-1, y0.shape[-1]), y1.reshape(-1, y1.shape[-1])]))
        out.append(dict(fixture=("layer_lg.npz" if (lg or an) else "layer.npz") + ":" + name, **head_metrics(ys[0], ys[1], seeded_head(ys[0].shape[-1], 7))))
        print(out[-1], flush=True)
    return out


def replay(fixture, pre, model_type, heads):
    """the recorded calls `pre`call<j>.* of a drafting loop through a seeded model in both formats; metrics over the rows of all calls"""
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    H, V = 256, 65536
    cfg = types.SimpleNamespace(vocab_size=V, hidden_size=H, pad_token_id=None, num_hidden_layers=1, num_attention_heads=heads, num_key_value_heads=heads,
                                intermediate_size=2 * H, max_position_embeddings=2048, rms_norm_eps=1e-5, model_parallel_size=1, input_type="t2i")
    torch.manual_seed(3)
    mdls = [cnets.Model(cfg, total_tokens=59, depth=5, top_k=10, model_type=model_type).to(dev).to(bf) for _ in range(2)]
    mdls[1].load_state_dict(mdls[0].state_dict())
    mdls[1].set_weight_format("fp8")
    n_calls = int(g[pre + "n_calls"])
    rows = [[], []]
    for mi, mdl in enumerate(mdls):
        gen = torch.Generator(device="cuda").manual_seed(11)
        kv = None
        for j in range(n_calls):
            ids = torch.from_numpy(g[pre + f"call{j}.ids"]).to(dev)
            pos = torch.from_numpy(g[pre + f"call{j}.pos"]).to(dev)
            past = int(g[pre + f"call{j}.past"])
            B, T = ids.shape
            key = pre + f"call{j}.attn"
            am = torch.from_numpy(g[key] if key in g.files else g[pre + "attn"]).to(dev).bool()
            if am.shape[1] < past + T:          # the loop extends the mask by ones for the tokens behind the prompt
                am = torch.cat([am, torch.ones(B, past + T - am.shape[1], dtype=torch.bool, device=dev)], dim=1)
            am = am[:, :past + T]
            key = pre + f"call{j}.tree"
            tree = g[key] if key in g.files and g[key].size else None
            mdl.tree_mask = None if tree is None else torch.from_numpy(tree).to(dev).float()
            hid = torch.randn(B, T, H, device=dev, dtype=bf, generator=gen)
            past_kv = None if (kv is None or past == 0) else tuple((k[:, :, :past], v[:, :, :past]) for k, v in kv)
            with torch.no_grad():
                y, kv = mdl(hid, ids, attention_mask=am, position_ids=pos, past_key_values=past_kv, use_cache=True)
            live = am[:, past:past + T].reshape(-1)          # (padding rows carry no proposal)
            rows[mi].append(y.reshape(B * T, H)[live])
        mdl.reset_kv()
    out = dict(fixture=fixture + ":" + pre.rstrip("."), calls=n_calls, **head_metrics(torch.cat(rows[0]), torch.cat(rows[1]), seeded_head(H, 9)))
    print(out, flush=True)
    return out


res = layer_fixtures()
for fixture, model_type, heads in (("lumina_drafter.npz", "lumina_mgpt", 2), ("anole_drafter.npz", "anole", 4)):
    g = np.load(os.path.join(ROOT, "tests", "golden", fixture))
    for pre in sorted({k.split(".")[0] + "." for k in g.files if k.endswith(".n_calls")}):
        try:
            res.append(replay(fixture, pre, model_type, heads))
        except (cnets.ops._lib.LanternError, ValueError, IndexError, AssertionError) as e:          # a recorded call the kernels refuse (host-side check): reported, not hidden
            res.append(dict(fixture=fixture + ":" + pre.rstrip("."), error=f"{type(e).__name__}: {e}"))
            print(res[-1], flush=True)
print(json.dumps(res))
if len(sys.argv) > 1:
    json.dump(res, open(sys.argv[1], "w"), indent=1)
