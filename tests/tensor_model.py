"""Model of the tensor output (mij_batch_set_out_tensor / TensorDecoder) on the CPU: crop window, flips, layout and per-channel table
applied to reference pixels (golden vectors or the oracle).  Used as the expected value of the GPU tests."""
import numpy as np
import torch

BITS = {torch.uint8: torch.uint8, torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32}
ESIZE = {torch.uint8: 1, torch.float16: 2, torch.bfloat16: 2, torch.float32: 4}
CODE = {torch.uint8: 0, torch.float16: 1, torch.bfloat16: 2, torch.float32: 3}


def tables(n, dtype, mean=None, std=None):
    """the documented contract, restated: ((arange(256) / 255 - mean[c]) / std[c]) cast to dtype; v / 255 without mean / std"""
    if dtype == torch.uint8:
        return torch.arange(256, dtype=torch.int64).to(torch.uint8).repeat(n, 1)
    v = torch.arange(256, dtype=torch.float32) / 255
    rows = []
    for c in range(n):
        m = 0.0 if mean is None else float(mean[c])
        s = 1.0 if std is None else float(std[c])
        rows.append(((v - m) / s).to(dtype) if (mean is not None or std is not None) else v.to(dtype))
    return torch.stack(rows)


def window(px, win, flip_x=False, flip_y=False, layout="CHW", table=None, dtype=torch.uint8):
    """px: uint8 [H, W, C] numpy; -> torch tensor [C, h, w] or [h, w, C] of dtype"""
    if px.ndim == 2:
        px = px[:, :, None]
    x0, y0, w, h = win
    a = np.ascontiguousarray(px[y0:y0 + h, x0:x0 + w])
    if flip_x:
        a = a[:, ::-1]
    if flip_y:
        a = a[::-1]
    v = torch.from_numpy(a.copy()).long()
    if table is None:
        o = v.to(torch.uint8)
    else:
        o = torch.stack([table[c][v[..., c]] for c in range(v.shape[-1])], -1)
    return o.permute(2, 0, 1).contiguous() if layout == "CHW" else o.contiguous()


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(BITS[a.dtype]), b.contiguous().view(BITS[b.dtype]))
