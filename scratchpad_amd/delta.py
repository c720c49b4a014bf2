"""The packed format of a delta topping: W_finetuned - W_base stored 4-bit and 2:4 sparse (include/scratchpad_hip.h
states the layout sp_delta_mm reads; this module is its definition in plain torch on CPU tensors).

For a dense delta D [N, K] (output rows x input width), every run of 4 consecutive columns keeps 2 positions p0 < p1:

    codes  uint8 [N, K / 4]   byte g of row n: low nibble = the code at p0, high nibble = the code at p1 of group g
    meta   uint8 [N, K / 8]   byte m: group 2 m in the low, group 2 m + 1 in the high nibble; a nibble is p0 | p1 << 2
    scales [N]                fp16 / bf16, one per output row;  D[n, 4 g + p] = scales[n] * (code - 8)

How a fine-tune is best compressed into this form (deltazip's algorithm) is not this module's concern: ``pack_delta`` is
round-to-nearest magnitude pruning, enough to produce and to test the format.  Converting a deltazip checkpoint (whose
buffers are in triteia's Marlin tile order) is out of scope."""
from typing import Optional, Tuple

import torch

ZERO_CODE = 0x88        # a code byte of two zeros (code 8 at both kept positions)
ZERO_META = 0x44        # a meta byte of two groups that keep positions 0 and 1


def _check_shape(N: int, K: int) -> None:
    if K <= 0 or K % 8 != 0 or N <= 0:
        raise ValueError(f"a packed delta needs N > 0 rows and K a positive multiple of 8 columns, got [{N}, {K}]")


def pack_delta(D: torch.Tensor, dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(codes, meta, scales) of the dense delta D [N, K].  Per group of 4 columns the 2 largest magnitudes are kept
    (ties: the lower column); scale[n] = max |kept| / 7 rounded to ``dtype`` (D's own when it is fp16 / bf16), 1 for a
    row that is all zero (or whose scale rounds to 0); code = round-to-nearest(value / scale) clamped to [-8, 7], + 8.
    Canonical form: a kept value that rounds to code 8 (zero) gives its position up to the lowest free column of the
    group, so that the packed tensors are a function of the dense matrix ``unpack_delta`` returns."""
    if D.dim() != 2:
        raise ValueError("pack_delta takes a dense [N, K] matrix")
    if dtype is None:
        dtype = D.dtype if D.dtype in (torch.float16, torch.bfloat16) else torch.bfloat16
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"scales are fp16 or bf16, not {dtype}")
    N, K = D.shape
    _check_shape(N, K)
    d = D.detach().cpu().double().view(N, K // 4, 4)

    def top2(mag):
        order = torch.sort(mag, dim=-1, descending=True, stable=True).indices[..., :2]
        return order.min(-1).values, order.max(-1).values

    p0, p1 = top2(d.abs())
    kept = torch.stack([d.gather(-1, p0.unsqueeze(-1)).squeeze(-1), d.gather(-1, p1.unsqueeze(-1)).squeeze(-1)], -1)
    scale = (kept.abs().amax(dim=(1, 2)) / 7.0).to(dtype)
    scale = torch.where(scale.double() > 0, scale, torch.ones_like(scale))
    q = torch.round(kept / scale.double().view(N, 1, 1)).clamp_(-8, 7)
    # canonical positions: by the magnitude of what is stored
    dense_q = torch.zeros(N, K // 4, 4, dtype=torch.float64)
    dense_q.scatter_(-1, torch.stack([p0, p1], -1), q)
    p0, p1 = top2(dense_q.abs())
    c0 = dense_q.gather(-1, p0.unsqueeze(-1)).squeeze(-1).long() + 8
    c1 = dense_q.gather(-1, p1.unsqueeze(-1)).squeeze(-1).long() + 8
    codes = (c0 | (c1 << 4)).to(torch.uint8)
    nib = (p0 | (p1 << 2)).view(N, K // 8, 2)
    meta = (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8)
    return codes.contiguous(), meta.contiguous(), scale.contiguous()


def unpack_delta(codes: torch.Tensor, meta: torch.Tensor, scales: torch.Tensor,
                 dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """the dense D [N, K] of a packed delta, scales[n] * (code - 8) at the kept positions (exact in fp32), on the
    device of its arguments"""
    if codes.dim() != 2 or meta.dim() != 2 or scales.dim() != 1 or codes.dtype != torch.uint8 \
            or meta.dtype != torch.uint8:
        raise ValueError("unpack_delta takes codes uint8 [N, K / 4], meta uint8 [N, K / 8] and scales [N]")
    N, G = codes.shape
    _check_shape(N, 4 * G)
    if tuple(meta.shape) != (N, G // 2) or scales.shape[0] != N:
        raise ValueError(f"codes {tuple(codes.shape)}, meta {tuple(meta.shape)} and scales {tuple(scales.shape)} do "
                         "not belong to one matrix")
    c = codes.long()
    m = meta.long()
    nib = torch.stack([m & 15, m >> 4], -1).view(N, G)
    p0, p1 = nib & 3, nib >> 2
    if bool((p0 >= p1).any()):
        raise ValueError("a meta nibble must name two positions p0 < p1")
    q = torch.zeros(N, G, 4, dtype=torch.float32, device=codes.device)       # integers in [-8, 7]
    q.scatter_(-1, torch.stack([p0, p1], -1), torch.stack([(c & 15) - 8, (c >> 4) - 8], -1).float())
    return (q.view(N, 4 * G) * scales.float().view(N, 1)).to(dtype)             # 4-bit x 11-bit: exact in fp32


def empty_delta(N: int, K: int, dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the packed form of an all-zero [N, K] delta: code 8 everywhere, scale 1"""
    _check_shape(N, K)
    return (torch.full((N, K // 4), ZERO_CODE, dtype=torch.uint8), torch.full((N, K // 8), ZERO_META, dtype=torch.uint8),
            torch.ones(N, dtype=dtype))
