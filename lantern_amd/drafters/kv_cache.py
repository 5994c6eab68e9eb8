"""KV-cache bookkeeping with the reference's API (models/drafters/kv_cache.py:4-155).

Layout contract kept: one slab per device `[2*L, B, Hkv, max_position_embeddings, head_dim]`,
per-layer K/V views, `current_length` as a CPU int64 tensor `[2L]` (the reference keeps it on the
host "for quick access", kv_cache.py:124-128).  `KVCache.copy` -- the accepted-path move -- runs
the HIP gather (`lantern_kv_gather`) instead of index_select + copy_.

`kv_format="fp8"` (opt-in): the slab holds FP8 rows (include/lantern_hip.h, "FP8 KV cache") -- uint8
`[2*L, B, Hkv, max_position_embeddings, head_dim + 16]`; `cat` quantises the new rows in place
(`lantern_kv8_append`), `copy` moves the byte rows with the same gather, `ops.tree_attention` reads them.
"""
from __future__ import annotations

import torch


class KVCache:
    def __init__(self, data: torch.Tensor, current_length: torch.Tensor):
        self.data = data
        self.current_length = current_length

    @property
    def fp8(self) -> bool:
        return self.data.dtype == torch.uint8

    @property
    def shape(self):
        return (self.data.shape[0], self.data.shape[1], self.current_length.item(), self.data.shape[3] - (16 if self.fp8 else 0))

    def copy(self, indices: torch.Tensor, prev_length: int, dim: int = 2):
        from .. import ops
        assert dim == 2, "KV slabs gather along the sequence axis"
        n = indices.numel()
        dev = self.data.device
        retrieve = (indices.to(torch.int64) - prev_length).reshape(1, n).to(dev)
        best = torch.zeros(1, dtype=torch.int32, device=dev)
        alen = torch.full((1,), n - 1, dtype=torch.int32, device=dev)
        ops.kv_gather([self.data], torch.zeros(1, dtype=torch.int32, device=dev),
                      torch.tensor([prev_length], dtype=torch.int64, device=dev), retrieve, best, alen)
        self.current_length.fill_(prev_length + n)

    def cat(self, tensor: torch.Tensor, dim: int = 2):
        if self.fp8:
            from .. import ops
            assert dim == 2, "KV slabs grow along the sequence axis"
            if int(self.current_length) + tensor.shape[2] > self.data.shape[2]:
                raise ValueError(f"KVCache.cat: {tensor.shape[2]} rows behind {int(self.current_length)} do not fit {self.data.shape[2]}")
            ops.kv8_append(tensor, None, self.data, None, int(self.current_length))
            self.current_length.add_(tensor.shape[2])
            return torch.narrow(self.data, 2, 0, int(self.current_length))
        dst = self.data.narrow(dim, int(self.current_length), tensor.shape[dim])
        dst.copy_(tensor)
        self.current_length.add_(tensor.shape[dim])
        return torch.narrow(self.data, 2, 0, int(self.current_length))


def initialize_past_key_values(model, batch_size: int = 1, kv_format: str = "bf16"):
    """Same return triple as the reference: (past_key_values, [slabs], current_length_data).
    Single-device form (the multi-device split of kv_cache.py:88-122 belongs to the out-of-scope
    model-parallel loader).  kv_format "bf16": the model's dtype, as the reference; "fp8": FP8 rows (uint8, head_dim + 16 bytes each)."""
    if kv_format not in ("bf16", "fp8"):
        raise ValueError(f"initialize_past_key_values: kv_format {kv_format!r} (\"bf16\" or \"fp8\")")
    config = model.config
    try:
        device = model.model.layers[0].self_attn.q_proj.weight.device
    except AttributeError:
        device = next(model.parameters()).device
    L = config.num_hidden_layers
    if kv_format == "fp8":
        from .. import ops
        d = config.hidden_size // config.num_attention_heads
        row = ops.kv8_row_bytes(d)
        if not row:
            raise ValueError(f"initialize_past_key_values: no FP8 row format for head_dim {d} (64 or 128)")
        data = torch.zeros(L * 2, batch_size, config.num_key_value_heads, config.max_position_embeddings, row, device=device, dtype=torch.uint8)
    else:
        data = torch.zeros(L * 2, batch_size, config.num_key_value_heads, config.max_position_embeddings,
                           config.hidden_size // config.num_attention_heads, device=device, dtype=model.dtype)
    current_length_data = torch.zeros(L * 2, dtype=torch.long, device="cpu")
    past_key_values = [[KVCache(data[2 * i + j], current_length_data[2 * i + j]) for j in range(2)] for i in range(L)]
    return past_key_values, [data], current_length_data
