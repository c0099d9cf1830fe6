"""
Cases, inputs and references of the exact, every-route tests of the dJPEG rate term (csrc/djpeg_entropy.hip):
tests/test_gpu_djpeg_rate_exact.py runs the kernels, tests/test_djpeg_rate_cases.py proves on the CPU the conditions these references
have to meet.  Nothing here needs a GPU.

The reference starts from z = X / Q of the C oracle (oracle/djpeg_ref.c djpeg_ref_forward_z), the float32 value the kernels form bit
for bit, never from x: a float32 z of several hundred seen through a kernel of width 1 / 25 is what made the end-to-end tolerances
of tests/djpeg_entropy_ref.py 1e-3 .. 3.4e-2.  From that z on everything is float64:

    e    = quantise(mode, z)     rint for round / soft, z for identity, the formula of djpeg.h in float64 rounded to float32 for
                                 sin / harmonic (the kernel's e is a float32)
    hm_k = mean_i wn_k(e_i)      over ALL 512 centres (djpeg_entropy_ref.full_weights' definition), on the distinct bit patterns of
                                 e and their counts, a chunk of values at a time
    H, g_k = dH / d hm_k         1e-9 clip, re-normalisation, / 0.6931
    G    = coef / N * sum_k g_k d wn_k / d e * surrogate(mode, z) / Q
    dq   = [-sum G z (Y), -sum G z (Cb + Cr)],   gx = the float64 adjoint of x -> X applied to G (torch autograd)

A batch is (base images, index): image i of the batch is base[index[i]].  The estimator pools the whole batch, everything else is
per image, so a tiled batch (grid-cap: 2056 images, 7 distinct) costs what its distinct images cost.
"""
import functools
import math

import numpy as np
import torch

import djpeg_cases as C
import djpeg_sub_ref as S
from djpeg_entropy_ref import CODEBOOK, EPS, GAMMA, HI, LO, V
from oracle import tables as ot

MODES = ('round', 'soft', 'sin', 'harmonic', 'identity')
EXACT_E = ('round', 'soft', 'identity')            # modes whose e carries no device rounding of its own
MAX_GRID, SEGS, WAVES = 1024, 32, C.WAVES
CLIP = 1e-9
CHUNK = 2048                                       # values per (CHUNK, 512) float64 block

# id -> (n, h, w)
CASES = dict(C.CASES)
CASES.update({
    'seg-31': (124, 8, 8),            # 31 workgroups: every segment sum is one partial or none
    'seg-32': (125, 8, 8),            # 32 workgroups, the last with one live wave: every segment exactly one partial
    'seg-33': (129, 8, 8),            # 33 workgroups: segment 0 is the first to sum two partials
    'grid-cap': (2056, 8, 72),        # 4112 tasks on the capped grid of 1024: the 16 waves of workgroups 0 .. 3 run two tasks
    'codebook-sweep': (1, 128, 128),  # the ends of the code book, the switch to the 512-centre loop, the zero-centre registers
})
ROUTE_CASES = C.CASE_IDS + ['seg-31', 'seg-32', 'seg-33']
GRID_CAP_PERIOD = 7                   # coprime to every stride of the task walk (2, 4, 4096): a wrong task meets other content

# hardware cosine of quantise_grad: four times what the same surrogate measured in djpeg_bwd_kernel (of max|ref|)
A_GX, A_DQ = 4 * 9.2e-6, 4 * 2.6e-5
TINY = 2.0 ** -126                    # below the smallest normal float32 a result carries absolute, not relative, precision
G_TOL_EXACT = 1e-10                   # float64 arithmetic sits near 1e-13, one lost or doubled value moves a bin by >= 2.8e-7


def tasks_of(shape):
    return C.tasks_of(shape)


def grid_of(shape):
    return min(MAX_GRID, (tasks_of(shape) + WAVES - 1) // WAVES)


def waves_with_two_tasks(shape):
    return max(0, tasks_of(shape) - WAVES * grid_of(shape))


# ------------------------------------------------------------------------------------------------------------------------------
# tables and inputs
SWEEP_DC = {'sweep-int': 4.0, 'sweep-frac': 3.96}


def table(name):
    """djpeg_cases.table plus the two tables of codebook-sweep: IJG q50 with the three DC entries at 4 (every entry an integer: the
    Markstein route) or at 3.96 (the IEEE route).  A flat grey block of level j / 255 has the luma DC 8.0017 (j - 127): over 4 it
    sweeps -254.05 .. 256.05 (nearest centres 1 .. 511, all in range), over 3.96 it sweeps -256.6 .. 258.6: j = 0 below the range,
    j = 1 at -254.6 (centre 0), j = 253 at 254.6 (centre 510), j = 254 and 255 - neighbours in the last strip - above it.  The
    chroma DCs of the saturated-colour blocks leave the range at both ends too (+-257.1 over 4, +-259.7 over 3.96).  No value lies
    7 or more beyond the book, where eps = 1e-72 outweighs every kernel weight and the value spreads 1 / 512 on each bin."""
    if name in SWEEP_DC:
        q = C.ijg(50)
        q[:, 0, 0] = SWEEP_DC[name]
        return q
    return C.table(name)


_SATURATED = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 0.5, 0), (0, 0.5, 1)]


def sweep_image():
    """(1, 128, 128, 3): block j of the 16 x 16 (raster order, so levels 0 .. 7 share the first strip and 248 .. 255 the last) is
    grey level j / 255; blocks 96 .. 111 carry saturated colours instead, so that the chroma DCs leave their rest value.  On top,
    the same zero-mean texture in every block (per channel, +-0.2): the DCs stay the sweep, and a tenth of the values and more
    leave the zero centre."""
    rng = np.random.default_rng(128128)
    tex = rng.uniform(-0.2, 0.2, (8, 8, 3))
    tex -= tex.mean(axis=(0, 1), keepdims=True)
    blocks = np.zeros((16, 16, 8, 8, 3))
    for j in range(256):
        colour = _SATURATED[(j - 96) % 8] if 96 <= j < 112 else (j / 255.0,) * 3
        blocks[j // 16, j % 16] = np.asarray(colour)[None, None, :] + tex
    return blocks.transpose(0, 2, 1, 3, 4).reshape(1, 128, 128, 3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch(case, kind):
    """(base (m, h, w, 3) float32, index (n,)): image i of the batch is base[index[i]].  Read-only."""
    n, h, w = CASES[case]
    if case == 'codebook-sweep':
        base, index = sweep_image(), np.zeros(1, np.int64)
    elif case == 'grid-cap':
        base, index = C.images((GRID_CAP_PERIOD, h, w), kind), np.arange(n) % GRID_CAP_PERIOD
    else:
        base, index = C.images((n, h, w), kind), np.arange(n)
    base.setflags(write=False)
    index.setflags(write=False)
    return base, index


def inputs(case, kind):
    base, index = batch(case, kind)
    return base[index]


# Tables of ones on a saturated image: |z| up to ~700.  A value 7 or more beyond the code book weighs under eps = 1e-72 at every
# centre and spreads 1 / 512 on each bin; with N < 1 / (512e-9) = 1.95 M values that alone lifts every bin over the 1e-9 clip.  It is
# the one run without a clipped bin (tests/test_djpeg_rate_cases.py proves both halves); the noise inputs under `ones` stay near the
# range and keep clipped bins.
FAR_RUN = ('three-strips', 'saturated', 'ones')
FAR_BEYOND = 7.0


# (case, input, table, mode)
def _runs():
    runs = []
    for case in ROUTE_CASES:
        for mode in MODES:
            runs += [(case, 'saturated', 'q50', mode), (case, 'noise', 'frac', mode)]
    for mode in MODES:
        runs += [('one-block', 'noise', 'ones', mode), ('full+ragged', 'noise', 'ones', mode)]
        runs += [('three-strips', 'noise', 'q95', mode), ('full', 'noise', 'q95', mode)]
    runs += [FAR_RUN + (mode,) for mode in MODES]
    runs += [('full+ragged', 'saturated', 'last', mode) for mode in MODES]
    runs += [('codebook-sweep', 'sweep', tab, mode) for tab in SWEEP_DC for mode in MODES]
    runs += [('grid-cap', 'saturated', 'q50', mode) for mode in ('round', 'sin', 'identity')]
    return runs


RUNS = _runs()
RUN_IDS = ['-'.join(r) for r in RUNS]


# ------------------------------------------------------------------------------------------------------------------------------
# the quantiser and its surrogate
def quantise(mode, z):
    """e (float32) of a float32 z."""
    z = np.asarray(z)
    assert z.dtype == np.float32
    if mode in ('round', 'soft'):
        return np.rint(z)
    if mode == 'identity':
        return z.copy()
    z64 = z.astype(np.float64)
    s = np.sin(2.0 * np.pi * (z64 - np.rint(z64)))
    return (z64 - s / (2.0 * np.pi if mode == 'sin' else np.pi)).astype(np.float32)


def surrogate(mode, z):
    z64 = np.asarray(z, np.float64)
    if mode == 'round':
        return np.zeros_like(z64)
    if mode == 'identity':
        return np.ones_like(z64)
    c = np.cos(2.0 * np.pi * (z64 - np.rint(z64)))
    return 1.0 - c if mode in ('soft', 'sin') else 1.0 - 2.0 * c


# ------------------------------------------------------------------------------------------------------------------------------
# the estimator over all 512 centres
def _weights(u):
    """(w + eps (len(u), 512), d w / d u) of float64 values u."""
    assert (V, GAMMA) == (50.0, 25.0)
    t = GAMMA * (u[:, None] - CODEBOOK[None, :])
    base = 1.0 + t * t / V
    b8 = ((base * base) ** 2) ** 2
    w0 = 1.0 / (b8 * b8 * b8 * base * np.sqrt(base))             # base ** -25.5 (np.power is several times slower)
    return w0 + EPS, w0 * (-(V + 1.0) / V * GAMMA) * t / base


def histogram_sum(u, counts):
    """sum_i counts_i wn_k(u_i), (512,)."""
    acc = np.zeros(CODEBOOK.size)
    for a in range(0, u.size, CHUNK):
        w, _ = _weights(u[a:a + CHUNK])
        acc += (counts[a:a + CHUNK, None] * (w / w.sum(axis=1, keepdims=True))).sum(axis=0)
    return acc


def finalize(hm):
    """(H, g_k = dH / d hm_k) of the mean histogram: clip at 1e-9, re-normalise, / 0.6931; no gradient through an active clip."""
    clipped = hm < CLIP
    hc = np.where(clipped, CLIP, hm)
    T = hc.sum()
    q = hc / T
    lq = np.log(q)
    H = -(q * lq).sum() / 0.6931
    g = np.where(clipped, 0.0, (-(lq + 1.0) + (q * (lq + 1.0)).sum()) / T / 0.6931)
    return H, g


def dde(u, g):
    """sum_k g_k d wn_k / d u at every u: (A - B dS / S) / S."""
    out = np.empty(u.size)
    for a in range(0, u.size, CHUNK):
        w, dw = _weights(u[a:a + CHUNK])
        Ssum, dS = w.sum(axis=1), dw.sum(axis=1)
        out[a:a + CHUNK] = (dw @ g - (w @ g) * dS / Ssum) / Ssum
    return out


def estimator(e, weight=None):
    """e: float32 array; weight: how often each element counts (same shape; None: once).
    -> dict(H, g (512,), hm (512,), dde (shape of e, per value, NOT divided by N), N)."""
    bits = np.ascontiguousarray(e, np.float32).view(np.uint32).reshape(-1)
    ub, inv = np.unique(bits, return_inverse=True)
    inv = inv.reshape(-1)
    counts = np.bincount(inv, weights=None if weight is None else np.asarray(weight, np.float64).reshape(-1),
                         minlength=ub.size).astype(np.float64)
    u = ub.view(np.float32).astype(np.float64)
    N = counts.sum()
    hm = histogram_sum(u, counts) / N
    H, g = finalize(hm)
    return dict(H=H, g=g, hm=hm, dde=dde(u, g)[inv].reshape(np.shape(e)), N=N, distinct=int(ub.size))


def estimator_plain(e):
    """The same without np.unique: every value on its own (small inputs only)."""
    u = np.asarray(e, np.float32).astype(np.float64).reshape(-1)
    hm = histogram_sum(u, np.ones(u.size)) / u.size
    H, g = finalize(hm)
    return dict(H=H, g=g, hm=hm, dde=dde(u, g).reshape(np.shape(e)), N=float(u.size))


# ------------------------------------------------------------------------------------------------------------------------------
# the linear part x -> X and its adjoint
def linear_X(x):
    """The linear part of djpeg_cases.restate64: (n, h, w, 3) -> X (n, 3, h/8, w/8, 8, 8), in x's dtype."""
    dt = x.dtype
    cf = torch.tensor(ot.COLOR_F, dtype=dt)
    Fm = torch.tensor(ot.DCT_F, dtype=dt)
    xc = torch.cat([torch.ones_like(x[..., :1]), 255.0 * x], dim=-1)
    ycc = xc @ cf.t() - 127
    return torch.stack([Fm @ S._blocks(ycc[..., c]) @ Fm.t() for c in range(3)], dim=1)


def adjoint(G, shape, dtype=torch.float64):
    """d sum(X * G) / d x by autograd, at `dtype`; G (m, 3, hb, wb, 8, 8), shape (m, h, w, 3)."""
    x = torch.zeros(shape, dtype=dtype, requires_grad=True)
    cot = torch.as_tensor(np.ascontiguousarray(G)).to(dtype)
    (gx,) = torch.autograd.grad(linear_X(x), x, cot)
    return gx.numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference of a run
def _gradients(z, q, mode, est, coef, mult_e, shape):
    """(G, gx of the base images, dq (2, 8, 8)) from the estimator's dde."""
    z64 = z.astype(np.float64)
    G = coef / est['N'] * est['dde'] * surrogate(mode, z) / q.astype(np.float64)[None, :, None, None, :, :]
    d3 = -(G * z64 * mult_e).sum(axis=(0, 2, 3))
    return G, adjoint(G, shape), np.stack([d3[0], d3[1] + d3[2]])


def _rel(diff, ref):
    m = np.abs(ref).max()
    return float(np.abs(diff).max() / m) if m > 0 else 0.0


def reference_from(base, index, q, mode, coef=1.0):
    """The float64 reference and the floors of its comparison with the kernels: dict(
         z, e (of the base images), H, g, hm, gx (of the base images: the batch's is gx[index]), dq, distinct,
         F_t_gx, F_t_dq   the linear adjoint in float32 against float64 on the same cotangent, of max|ref|,
         F_e_*            the largest change when every e moves to its float32 neighbour, all up / all down (0 for the exact-e modes),
         tol_g, tol_H (absolute), tol_gx, tol_dq (of max|ref|))."""
    z = C.c_forward_z(base, q)['z']
    mult = np.bincount(index, minlength=base.shape[0]).astype(np.float64)
    mult_e = mult[:, None, None, None, None, None]
    weight = np.broadcast_to(mult_e, z.shape)
    e = quantise(mode, z)
    est = estimator(e, weight)
    G, gx, dq = _gradients(z, q, mode, est, coef, mult_e, base.shape)
    out = dict(z=z, e=e, H=est['H'], g=est['g'], hm=est['hm'], gx=gx, dq=dq, distinct=est['distinct'], N=est['N'])
    # F_t: float32 against float64, same cotangent
    out['F_t_gx'] = _rel(adjoint(G.astype(np.float32), base.shape, torch.float32) - gx, gx)
    # (for dq the float32 sum runs over the images of the BATCH, as the kernels' does: 2056 terms deep in grid-cap, not 7 weighted)
    terms = torch.from_numpy(G.astype(np.float32)) * torch.from_numpy(z)
    d32 = -terms[torch.from_numpy(np.array(index))].sum(dim=(0, 2, 3)).numpy().astype(np.float64)
    out['F_t_dq'] = _rel(np.stack([d32[0], d32[1] + d32[2]]) - dq, dq)
    # F_e: what the device's sinpif may cost
    F = dict(g=0.0, H=0.0, gx=0.0, dq=0.0)
    if mode not in EXACT_E:
        for towards in (np.float32(np.inf), np.float32(-np.inf)):
            est_s = estimator(np.nextafter(e, towards), weight)
            _, gx_s, dq_s = _gradients(z, q, mode, est_s, coef, mult_e, base.shape)
            F['g'] = max(F['g'], _rel(est_s['g'] - est['g'], est['g']))
            F['H'] = max(F['H'], abs(est_s['H'] - est['H']))
            F['gx'] = max(F['gx'], _rel(gx_s - gx, gx))
            F['dq'] = max(F['dq'], _rel(dq_s - dq, dq))
    for k, v in F.items():
        out['F_e_' + k] = v
    smooth_surrogate = mode in ('soft', 'sin', 'harmonic')
    out['tol_g'] = G_TOL_EXACT if mode in EXACT_E else 4 * F['g']
    out['tol_H'] = 2 * float(np.spacing(np.float32(abs(est['H'])))) + 4 * F['H']
    out['tol_gx'] = 4 * (out['F_t_gx'] + F['gx']) + (A_GX if smooth_surrogate else 0.0)
    out['tol_dq'] = 4 * (out['F_t_dq'] + F['dq']) + (A_DQ if smooth_surrogate else 0.0)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(case, kind, tab, mode):
    """The reference of a run, computed once and shared by the tests that need it (read-only)."""
    base, index = batch(case, kind)
    return reference_from(base, index, table(tab), mode)


# ------------------------------------------------------------------------------------------------------------------------------
# where the values of a run sit in the code book
def nearest_centre(e):
    """k0 of the kernels: rint(e) + 255 clamped to 0 .. 511 (in-range values only make use of it)."""
    return np.clip(np.rint(np.asarray(e, np.float64)).astype(np.int64) + 255, 0, 511)


def in_range(e):
    e = np.asarray(e)
    return (e >= np.float32(LO)) & (e <= np.float32(HI))


def strips_with_two_out_of_range(e):
    """Number of (image, block row, strip of 8 blocks, channel, coefficient) at which two or more blocks are out of range: the
    lanes of one __ballot round."""
    n, c, hb, wb = e.shape[:4]
    out = ~in_range(e)
    pad = (-wb) % 8
    out = np.pad(out, ((0, 0), (0, 0), (0, 0), (0, pad), (0, 0), (0, 0)))
    per_strip = out.reshape(n, c, hb, (wb + pad) // 8, 8, 8, 8).sum(axis=4)
    return int((per_strip >= 2).sum())


def ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def describe(case, kind, tab, mode, ref):
    return ('{}: distinct {}, F_t gx {:.2e} dq {:.2e}, F_e g {:.2e} H {:.2e} gx {:.2e} dq {:.2e}, tol g {:.2e} H {:.2e} gx {:.2e} '
            'dq {:.2e}'.format('-'.join((case, kind, tab, mode)), ref['distinct'], ref['F_t_gx'], ref['F_t_dq'], ref['F_e_g'],
                               ref['F_e_H'], ref['F_e_gx'], ref['F_e_dq'], ref['tol_g'], ref['tol_H'], ref['tol_gx'],
                               ref['tol_dq']))


assert math.gcd(GRID_CAP_PERIOD, 2 * 4 * 4096) == 1
