"""The drafter's prompt prefill (first call of topK_generate: the whole prompt through cnets.Model.forward) at the 7B layer size: the HIP path
(drafter_fc slices, lantern_linear_rows_packed, head stage, block-causal lantern_tree_attention) against the same model on torch's ops
(F.linear = hipBLASLt, eager softmax attention under the additive mask), milliseconds per call between HIP events.
usage: prefill_bench.py [--weight-format bf16|fp8] [--input-stage] [prompt tokens=600] [reps=5]
(--weight-format fp8: from 129 rows the layer's GEMMs and the input stage run the tiled kernel's fp8 instances, one launch each -- lantern_linear_rows_packed_fmt,
lantern_drafter_fc_packed; 33 - 128 rows go through the stream-K kernel in blocks of 32 rows.
--input-stage: also time the input stage alone, fc(cat(embed[ids] * scale, hidden)) on the same rows, as "ms_input_stage" in the JSON line)"""
import json, os, sys, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from lantern_amd.drafters import cnets, decoder_layer


def _take_option(name, default, choices=None):
    """`--name value` anywhere on the command line (removed from sys.argv: the positional arguments keep their places)"""
    if name in sys.argv:
        i = sys.argv.index(name)
        v = sys.argv[i + 1]
        del sys.argv[i:i + 2]
        if choices and v not in choices:
            sys.exit(f"{name}: one of {choices}")
        return v
    return default


WEIGHT_FORMAT = _take_option("--weight-format", "bf16", ("bf16", "fp8"))
INPUT_STAGE = "--input-stage" in sys.argv
if INPUT_STAGE:
    sys.argv.remove("--input-stage")

T = int(sys.argv[1]) if len(sys.argv) > 1 else 600
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev, bf = torch.device("cuda"), torch.bfloat16
cfg = types.SimpleNamespace(vocab_size=65536, hidden_size=4096, pad_token_id=None, num_hidden_layers=1, num_attention_heads=32, num_key_value_heads=32,
                            intermediate_size=11008, max_position_embeddings=4096, rms_norm_eps=1e-5, model_parallel_size=1)
torch.manual_seed(0)
mdl = cnets.Model(cfg, total_tokens=59, depth=5, top_k=10, model_type="lumina_mgpt").to(dev).to(bf)
mdl.init_tree()
mdl.set_weight_format(WEIGHT_FORMAT)
x = torch.randn(2, T, 4096, device=dev, dtype=bf)
ids = torch.randint(4, 8000, (2, T), device=dev)
am = torch.ones(2, T, dtype=torch.bool, device=dev)
am[1, :9] = False


def run():
    mdl.reset_kv()
    mdl.tree_mask = None
    with torch.no_grad():
        return mdl(x, ids, attention_mask=am, use_cache=True)[0]


def timed():
    run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        y = run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, y


def timed_input_stage():
    """cnets.Model._input_stage alone on the prefill's rows (what forward runs in front of the layer)"""
    with torch.no_grad():
        mdl._input_stage(x, ids)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            mdl._input_stage(x, ids)
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


ms_hip, y_hip = timed()
extra = {"ms_input_stage": round(timed_input_stage(), 3)} if INPUT_STAGE else {}
for l in mdl.layers:
    l.fused = False
    l.inplace_cache = False
decoder_layer._hip_ok = lambda a, b: False
ms_torch, y_torch = timed()
w_bytes = sum(p.numel() * 2 for p in mdl.layers[0].parameters())
flops = 2 * 2 * T * (w_bytes // 2)
print(json.dumps({"rows": 2 * T, "weight_format": WEIGHT_FORMAT, "ms_hip": round(ms_hip, 3), "ms_torch_ops": round(ms_torch, 3), "layer_weight_MB": round(w_bytes / 1e6, 1),
                  "layer_gemm_TFLOPs_hip": round(flops / ms_hip / 1e9, 1), "max_abs_diff_valid_rows": float((y_hip[:, 9:].float() - y_torch[:, 9:].float()).abs().max()), **extra}))
