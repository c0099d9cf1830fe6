"""
The differentiable JPEG with chroma sub-sampling, restated in torch float64 from its definition.  Test
infrastructure: every step is an ordinary torch expression, so autograd gives the gradients of x and of the tables.

  colour (reference matrices on 255 x, - 127)  ->  Cb / Cr: the mean of each hs x vs group  ->  per 8x8 block: DCT (4-decimal
  matrix), / Q, rounding approximation, * Q, inverse DCT (Y at (h, w), Cb / Cr at (h / vs, w / hs))  ->  chroma up-sampled with
  libjpeg's triangle filter in float (down the columns, then along the rows)  ->  + 127, inverse colour, / 255, clip to [0, 1]

(hs, vs) = (1, 1) is the reference's model (oracle.djpeg.djpeg_torch): no down-sampling, no filter.
"""
import torch

from oracle import tables
from oracle.tfops import quantization


def _blocks(p):          # (n,h,w) -> (n,h/8,w/8,8,8)
    n, h, w = p.shape
    return p.reshape(n, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)


def _unblocks(b):        # inverse of _blocks
    n, hb, wb, _, _ = b.shape
    return b.permute(0, 1, 3, 2, 4).reshape(n, hb * 8, wb * 8)


def box_down(p, hs, vs):
    """(n,h,w) -> (n,h/vs,w/hs): the mean of each hs x vs group."""
    n, h, w = p.shape
    return p.reshape(n, h // vs, vs, w // hs, hs).mean(dim=(2, 4))


def triangle_up(p, axis):
    """Doubles `axis`: out[2i] = 3/4 in[i] + 1/4 in[i-1], out[2i+1] = 3/4 in[i] + 1/4 in[i+1]; beyond the extent: the edge sample."""
    p = p.movedim(axis, -1)
    prev = torch.cat([p[..., :1], p[..., :-1]], -1)
    nxt = torch.cat([p[..., 1:], p[..., -1:]], -1)
    out = torch.stack([0.75 * p + 0.25 * prev, 0.75 * p + 0.25 * nxt], -1).reshape(*p.shape[:-1], 2 * p.shape[-1])
    return out.movedim(-1, axis)


def triangle_up_adjoint(g, axis):
    """The hand-written adjoint of triangle_up: in[i] gathers (1/4, 3/4, 3/4, 1/4) of out[2i-1 .. 2i+2] with CLAMPED indices, so
    the edge samples collect the replicated taps.  What the backward kernel computes."""
    g = g.movedim(axis, -1)
    m = g.shape[-1]
    i = torch.arange(m // 2)
    taps = [(2 * i - 1).clamp(0, m - 1), 2 * i, 2 * i + 1, (2 * i + 2).clamp(0, m - 1)]
    out = 0.25 * g[..., taps[0]] + 0.75 * g[..., taps[1]] + 0.75 * g[..., taps[2]] + 0.25 * g[..., taps[3]]
    return out.movedim(-1, axis)


def upsample(p, hs, vs):
    """(n,h/vs,w/hs) -> (n,h,w): down the columns first (4:2:0), then along the rows."""
    if vs == 2:
        p = triangle_up(p, 1)
    if hs == 2:
        p = triangle_up(p, 2)
    return p


def component_path(p, q, mode, idx_override=None):
    """One component plane through the block path: (reconstructed plane, dequantised coefficients, indices), blocks (n,hb,wb,8,8)."""
    Fm = torch.tensor(tables.DCT_F, dtype=p.dtype)
    X = Fm @ _blocks(p) @ Fm.t()
    idx = quantization(X / q, mode) if idx_override is None else idx_override.to(p.dtype) + 0 * X
    Xd = idx * q
    return _unblocks(Fm.t() @ Xd @ Fm), Xd, idx


def djpeg_sub_torch(x, q, mode='soft', hs=2, vs=2, idx_override=None, clip=True):
    """x (n,h,w,3) in [0,1], q (3,8,8) tables for Y, Cb, Cr; x and q may be autograd leaves.  idx_override: optional (luma, Cb, Cr)
    index tensors that replace the rounding's output (the comparison of a float32 kernel at ITS indices).
    Returns (y, (Xd_luma (n,hb,wb,8,8), Xd_chroma (n,2,hcb,wcb,8,8)), (idx_luma, idx_chroma), pre-clip y)."""
    dt = x.dtype
    n, h, w, _ = x.shape
    assert (hs, vs) in ((1, 1), (2, 1), (2, 2)) and h % (8 * vs) == 0 and w % (8 * hs) == 0
    cf = torch.tensor(tables.COLOR_F, dtype=dt)
    ci = torch.tensor(tables.COLOR_I, dtype=dt)
    xc = torch.cat([torch.ones_like(x[..., :1]), 255.0 * x], dim=-1)
    ycc = xc @ cf.t() - 127
    planes = [ycc[..., 0], box_down(ycc[..., 1], hs, vs), box_down(ycc[..., 2], hs, vs)]
    rec, Xd, idx = [], [], []
    for c, p in enumerate(planes):
        r_, X_, i_ = component_path(p, q[c], mode, None if idx_override is None else idx_override[c])
        rec.append(r_); Xd.append(X_); idx.append(i_)
    full = torch.stack([rec[0], upsample(rec[1], hs, vs), upsample(rec[2], hs, vs)], -1)
    qc = torch.cat([torch.ones_like(full[..., :1]), full + 127], dim=-1)
    pre = (qc @ ci.t()) / 255.0
    y = torch.clamp(pre, 0, 1) if clip else pre
    return y, (Xd[0], torch.stack(Xd[1:], 1)), (idx[0], torch.stack(idx[1:], 1)), pre


def psnr(a, b):
    """PSNR (dB) of two images in [0, 1], over the whole batch."""
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * torch.log10(torch.tensor(1.0 / max(mse, 1e-20))).item()
