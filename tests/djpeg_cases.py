"""
Cases, inputs and references of the exact, every-route tests of the 4:4:4 differentiable JPEG (csrc/djpeg.hip) and of the clip
mask of the sub-sampled one (csrc/djpeg_sub.hip): tests/test_gpu_djpeg_exact.py runs the kernels, tests/test_djpeg_cases.py proves
on the CPU the conditions that these references have to meet.  Nothing here needs a GPU.

A wave task is one 8-row strip of up to 64 pixels, four tasks per workgroup: tasks = n * (h / 8) * ceil(w / 64).  CASES are the
smallest shapes at which the strip and task logic can go wrong.

Two references:
  * the C restatement in the canonical float32 order (oracle/djpeg_ref.c djpeg_ref_forward_ex): hard rounding, compared bit for bit;
  * the float64 restatement (restate64, the hs = vs = 1 case of tests/djpeg_sub_ref.djpeg_sub_torch with the dequantised
    coefficients kept in the graph): smooth modes and every gradient, through autograd.
"""
import ctypes
import os

import numpy as np
import torch

import djpeg_sub_ref as R
from oracle import tables as ot
from oracle.tfops import quantization
from util import bits_to_keep, clip_bits, to64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STRIP_PX, WAVES = 64, 4

# id -> (n, h, w)
CASES = {
    'one-block': (1, 8, 8),           # 1 task: 3 idle waves; 7 of 8 block lanes inactive
    'ragged-only': (2, 16, 56),       # 4 tasks: one strip of 7 blocks; image and block-row decode
    'full+ragged': (1, 8, 72),        # 2 tasks: a full strip, then a strip of one block; 2 idle waves
    'exact-strip': (1, 24, 64),       # 3 tasks: w == STRIP_PX; three block rows; 1 idle wave
    'three-strips': (3, 8, 136),      # 9 tasks: three strips, the last ragged; tasks % 4 == 1; three images
    'full': (2, 16, 128),             # 8 tasks: no idle wave and no ragged strip (the control)
}
TASKS = {'one-block': 1, 'ragged-only': 4, 'full+ragged': 2, 'exact-strip': 3, 'three-strips': 9, 'full': 8}
CASE_IDS = list(CASES)
INPUTS = ['saturated', 'noise']
SMOOTH_INPUTS = INPUTS + ['unclipped']
INT_TABLES = ['q10', 'q50', 'q95', 'ones']          # the integer route (Markstein division)
FRAC_TABLES = ['frac', 'last']                      # the IEEE-division route
TABLES = INT_TABLES + FRAC_TABLES
HARD_MODES = ['round', 'soft']
SMOOTH_MODES = ['sin', 'harmonic', 'identity']
MODES = HARD_MODES + SMOOTH_MODES

# sub-sampled kernels: (sub-sampling, shape)
SUB = {'4:2:2': (2, 1), '4:2:0': (2, 2)}
SUB_CASES = [('4:2:0', (1, 16, 16)), ('4:2:0', (2, 48, 80)), ('4:2:2', (2, 24, 80))]
SUB_IDS = ['{}-{}x{}x{}'.format(s, *shape) for s, shape in SUB_CASES]

CLIP_SHARE = (0.05, 0.60)       # share of clear mask bits every `saturated` case must have, in the C oracle's mask
EDGE_HARD, EDGE_SMOOTH = 1e-6, 1e-5     # distance of a pre-clip value from 0 or 1 below which a mask bit may be left out
EDGE_CAP = 1e-3                 # ... for at most this share of the bits of a case
TIE_WIDTH, TIE_CAP = 1e-3, 1e-2  # |z - (k + 1/2)| below which rint(z) may flip in float32; at most this share of a case


def tasks_of(shape):
    n, h, w = shape
    return n * (h // 8) * ((w + STRIP_PX - 1) // STRIP_PX)


def _seed(shape):
    n, h, w = shape
    return 1000 * n + 10 * h + w


def images(shape, kind):
    """(n, h, w, 3) float32.  saturated: 4 x 4 patches drawn from [-0.5, 1.5) plus noise, clipped to [0, 1] and rounded to k / 255 -
    about half of the patches sit on a rail, so the codec's ringing leaves [0, 1] at a quarter of the values.  noise: uniform
    [0, 1), the worst case for rounding ties.  unclipped: the saturated image before its clip, for the `identity` mode - that codec
    is lossless up to the 4-decimal DCT matrix, so it returns every rail pixel of a saturated image to within 1e-5 of the rail
    (3 - 4 % of the values, measured: tests/test_djpeg_cases.py), where float32 and float64 may clip differently; an input that
    leaves [0, 1] itself clips under `identity` without sitting on the edge."""
    n, h, w = shape
    rng = np.random.default_rng(_seed(shape) + (1 if kind == 'noise' else 0))
    if kind == 'noise':
        return rng.random((n, h, w, 3)).astype(np.float32)
    assert kind in ('saturated', 'unclipped')
    base = np.kron(rng.uniform(-0.5, 1.5, (n, h // 4, w // 4, 3)), np.ones((1, 4, 4, 1)))
    img = base + rng.normal(0, 0.05, (n, h, w, 3))
    if kind == 'unclipped':
        return img.astype(np.float32)
    return (np.round(np.clip(img, 0, 1) * 255) / 255).astype(np.float32)


def gradient(shape, seed=12):
    n, h, w = shape
    return np.random.default_rng(seed + _seed(shape)).uniform(-1, 1, (n, h, w, 3)).astype(np.float32)


def ijg(quality):
    return np.stack([ot.jpeg_qtable(quality, 0), ot.jpeg_qtable(quality, 1), ot.jpeg_qtable(quality, 1)]).astype(np.float32)


def frac_pair():
    """(luma, chroma) trained-looking tables: IJG q60 times uniform(0.7, 1.3) (tests/test_gpu_ops.py test_djpeg_trainable_tables)."""
    rng = np.random.default_rng(23)
    ql = (ot.jpeg_qtable(60, 0) * rng.uniform(0.7, 1.3, (8, 8))).astype(np.float32)
    qc = (ot.jpeg_qtable(60, 1) * rng.uniform(0.7, 1.3, (8, 8))).astype(np.float32)
    return ql, qc


def table(name):
    """(3, 8, 8) float32 tables for Y, Cb, Cr."""
    if name == 'ones':
        return np.ones((3, 8, 8), np.float32)
    if name == 'frac':
        ql, qc = frac_pair()
        return np.stack([ql, qc, qc])
    if name == 'last':                  # one non-integer, at the last of the 192 staged entries: the whole launch divides
        q = ijg(50)
        q[2, 7, 7] += 0.5
        return q
    return ijg(int(name[1:]))


def table_pair(name):
    """(luma, chroma) of a table both chroma channels share ('q50', 'frac', ...)."""
    q = table(name)
    assert np.array_equal(q[1], q[2])
    return q[0], q[1]


def is_integer_table(q):
    return bool(((q >= 1) & (q <= 255) & (q == np.rint(q))).all())


# ------------------------------------------------------------------------------------------------------------------------------
# the C oracle
_CLIB = [None]


def clib():
    if _CLIB[0] is None:
        path = os.path.join(ROOT, 'oracle', 'libdjpeg_ref.so')
        if not os.path.isfile(path):
            raise RuntimeError('oracle/libdjpeg_ref.so not built (make -C oracle, or __graft_entry__.build())')
        _CLIB[0] = ctypes.CDLL(path)
    return _CLIB[0]


def _vp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def c_forward(x, q):
    """djpeg_ref_forward (the entry point smoke() and bench.py load): (y, idx, xd)."""
    x = np.ascontiguousarray(x, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    n, h, w, _ = x.shape
    y = np.zeros_like(x)
    idx = np.zeros((n, 3, h // 8, w // 8, 8, 8), np.int16)
    xd = np.zeros((n, 3, h // 8, w // 8, 8, 8), np.float32)
    assert clib().djpeg_ref_forward(_vp(x), _vp(y), _vp(q), _vp(idx), _vp(xd), n, h, w) == 0
    return y, idx, xd


def c_forward_ex(x, q):
    """djpeg_ref_forward_ex: dict(y, idx, xd, pre, mask)."""
    x = np.ascontiguousarray(x, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    n, h, w, _ = x.shape
    out = dict(y=np.zeros_like(x), idx=np.zeros((n, 3, h // 8, w // 8, 8, 8), np.int16),
               xd=np.zeros((n, 3, h // 8, w // 8, 8, 8), np.float32), pre=np.zeros_like(x),
               mask=np.full((n, h, w), 0xff, np.uint8))
    rc = clib().djpeg_ref_forward_ex(_vp(x), _vp(out['y']), _vp(q), _vp(out['idx']), _vp(out['xd']), _vp(out['pre']),
                                     _vp(out['mask']), n, h, w)
    assert rc == 0
    return out


def c_forward_z(x, q):
    """djpeg_ref_forward_z: dict(y, idx, xd, z), z = X / Q in float32 before the rounding, (n, 3, h/8, w/8, 8, 8)."""
    x = np.ascontiguousarray(x, np.float32)
    q = np.ascontiguousarray(q, np.float32)
    n, h, w, _ = x.shape
    out = dict(y=np.zeros_like(x), idx=np.zeros((n, 3, h // 8, w // 8, 8, 8), np.int16),
               xd=np.zeros((n, 3, h // 8, w // 8, 8, 8), np.float32), z=np.full((n, 3, h // 8, w // 8, 8, 8), np.nan, np.float32))
    assert clib().djpeg_ref_forward_z(_vp(x), _vp(out['y']), _vp(q), _vp(out['idx']), _vp(out['xd']), _vp(out['z']), n, h, w) == 0
    return out


_HARD = {}


def hard_reference(case, kind, tab):
    """The C oracle's outputs for (case id, input, table name), computed once and left unchanged."""
    key = (case, kind, tab)
    if key not in _HARD:
        ref = c_forward_ex(images(CASES[case], kind), table(tab))
        for a in ref.values():
            a.setflags(write=False)
        _HARD[key] = ref
    return _HARD[key]


def clear_share(mask):
    """Share of clear bits among the three clip bits of every pixel."""
    return 1.0 - float(bits_to_keep(mask).mean())


def near_edge(pre, width):
    """Bits whose pre-clip value lies within `width` of 0 or 1: a float32 kernel may decide them the other way."""
    pre = np.asarray(pre, np.float64)
    return (np.abs(pre) <= width) | (np.abs(pre - 1.0) <= width)


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 restatement
def restate64(x, q, mode):
    """The model of djpeg_sub_ref.djpeg_sub_torch(..., hs = 1, vs = 1, clip = False), stated with the dequantised coefficients
    kept IN the graph (djpeg_sub_torch returns a stacked copy of the chroma ones, which autograd never reaches).
    x (n,h,w,3) and q (3,8,8) float64 tensors, possibly leaves.  -> (pre-clip y, [Xd_c (n,hb,wb,8,8)], [z_c = X_c / q_c])."""
    dt = x.dtype
    cf = torch.tensor(ot.COLOR_F, dtype=dt)
    ci = torch.tensor(ot.COLOR_I, dtype=dt)
    Fm = torch.tensor(ot.DCT_F, dtype=dt)
    xc = torch.cat([torch.ones_like(x[..., :1]), 255.0 * x], dim=-1)
    ycc = xc @ cf.t() - 127
    rec, Xd, z = [], [], []
    for c in range(3):
        X = Fm @ R._blocks(ycc[..., c]) @ Fm.t()
        z.append(X / q[c])
        Xd.append(quantization(z[c], mode) * q[c])
        rec.append(R._unblocks(Fm.t() @ Xd[c] @ Fm))
    full = torch.stack(rec, -1)
    qc = torch.cat([torch.ones_like(full[..., :1]), full + 127], dim=-1)
    return (qc @ ci.t()) / 255.0, Xd, z


_SMOOTH = {}


def smooth_reference(case, kind, tab, mode):
    """float64 forward of a smooth mode: dict(y, pre, mask), computed once."""
    key = (case, kind, tab, mode)
    if key not in _SMOOTH:
        pre = restate64(to64(images(CASES[case], kind)), to64(table(tab)), mode)[0].numpy()
        _SMOOTH[key] = dict(pre=pre, y=np.clip(pre, 0, 1), mask=clip_bits(pre))
    return _SMOOTH[key]


def pattern_mask(shape):
    """A different combination of the three channel bits at every pixel of a row of eight, (x + 2 y) % 8 - it tells the bits and
    the byte positions of the packed mask row apart - under garbage in bits 3 .. 7, which the backward pass must ignore."""
    n, h, w = shape
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    m = ((xx + 2 * yy) % 8) | (((5 * xx + 3 * yy + 1) % 32) << 3)
    return np.broadcast_to(m.astype(np.uint8), (n, h, w)).copy()


def backward_reference(x, gy, ql, qc, mode, mask):
    """Autograd of the float64 restatement WITHOUT its clip: loss = sum(pre * gy * mask bits), x and the two tables as leaves,
    q = [ql, qc, qc].  -> dict(gx (n,h,w,3), dq (2,8,8) [luma, Cb + Cr], allow (2,8,8), tie_share).
    allow: per table entry, the sum of |d loss / d Xd| over the coefficients whose z = X / Q lies within TIE_WIDTH of a
    half-integer - what a flip of rint(z) in float32 can move that entry by (hard modes only; the smooth ones have no rint)."""
    xt = to64(x).requires_grad_(True)
    tl, tc = to64(ql).requires_grad_(True), to64(qc).requires_grad_(True)
    pre, Xd, z = restate64(xt, torch.stack([tl, tc, tc]), mode)
    for t in Xd:
        t.retain_grad()
    (pre * to64(gy) * torch.from_numpy(bits_to_keep(mask))).sum().backward()
    gx = xt.grad.numpy() if xt.grad is not None else np.zeros(x.shape)
    allow = np.zeros((2, 8, 8))
    ties = total = 0
    for c in range(3):
        zc = z[c].detach().numpy()
        tie = np.abs(zc - np.floor(zc) - 0.5) <= TIE_WIDTH
        ties, total = ties + int(tie.sum()), total + tie.size
        gd = np.zeros_like(zc) if Xd[c].grad is None else np.abs(Xd[c].grad.numpy())
        allow[0 if c == 0 else 1] += np.where(tie, gd, 0.0).sum(axis=(0, 1, 2))
    return dict(gx=gx, dq=np.stack([tl.grad.numpy(), tc.grad.numpy()]), allow=allow, tie_share=ties / float(total))


# ------------------------------------------------------------------------------------------------------------------------------
# the sub-sampled model
SUB_RUNS = [(s, shape, mode, 'saturated') for s, shape in SUB_CASES for mode in MODES] + \
           [(s, shape, 'identity', 'unclipped') for s, shape in SUB_CASES]
SUB_RUN_IDS = ['{}-{}x{}x{}-{}-{}'.format(s, *shape, mode, kind) for s, shape, mode, kind in SUB_RUNS]


def edge_cap_holds(mode, kind):
    """Whether at most EDGE_CAP of the reference's pre-clip values may lie at the edge of [0, 1]: everywhere but under `identity`
    on the saturated input (see images())."""
    return not (mode == 'identity' and kind == 'saturated')


_SUB = {}


def sub_reference(sub, shape, mode, kind='saturated'):
    """float64 forward of the sub-sampled model at IJG q50: dict(x, pre, y, mask, idx), computed once."""
    key = (sub, shape, mode, kind)
    if key not in _SUB:
        hs, vs = SUB[sub]
        x = images(shape, kind)
        y, _, idx, pre = R.djpeg_sub_torch(to64(x), to64(ijg(50)), mode, hs, vs)
        _SUB[key] = dict(x=x, pre=pre.numpy(), y=y.numpy(), mask=clip_bits(pre.numpy()), idx=[i.numpy() for i in idx])
    return _SUB[key]


def sub_backward_reference(sub, shape, mode, kind, gy, mask):
    """gx by autograd of the sub-sampled restatement without its clip, at the given mask bits."""
    hs, vs = SUB[sub]
    xt = to64(images(shape, kind)).requires_grad_(True)
    pre = R.djpeg_sub_torch(xt, to64(ijg(50)), mode, hs, vs, clip=False)[3]
    (pre * to64(gy) * torch.from_numpy(bits_to_keep(mask))).sum().backward()
    return xt.grad.numpy() if xt.grad is not None else np.zeros(gy.shape)
