"""Restatement and case list of the dJPEG rate term, shared by test_djpeg_entropy_host.py and
test_gpu_djpeg_entropy.py.

Reference: e = oracle/djpeg.py djpeg_torch(x, mode=, q=)[2] (the quantiser's output, X / Q through the rounding approximation)
-> oracle/tfops.py entropy(e.ravel(), codebook) with the code book of Quantization(latent_bpf=9): the 512 integers -255 .. 256,
v = 50, gamma = 25 - under torch autograd, in float64 (or float32 up to e, to measure the float32 floor of a case).
The gradient of the tables is [g[0], g[1] + g[2]] of the (3,8,8) leaf: the chroma table serves Cb and Cr.

Also the numpy form of the five-centre window the kernels rest on (window_weights / full_weights).
"""
import functools

import numpy as np
import torch

from oracle import djpeg as odj
from oracle import tables as ot
from oracle import tfops as T

from util import natural_images

CODEBOOK = np.arange(-255, 257).astype(np.float64)          # 512 centres
V, GAMMA, EPS = 50.0, 25.0, 1e-72
LO, HI = -255.5, 256.5                                      # the range the five-centre window covers
MODES = ('soft', 'sin', 'harmonic')
VALUE_TOL = 1e-5                                            # LAT_TOL['entropy'] (tests/tail_cases.py)
GRAD_ATOL = 1e-9


def ijg(quality):
    return np.stack([ot.jpeg_qtable(quality, 0), ot.jpeg_qtable(quality, 1), ot.jpeg_qtable(quality, 1)]).astype(np.float32)


def noninteger_tables():
    """test_djpeg_trainable_tables' recipe (tests/test_gpu_ops.py)."""
    rng = np.random.default_rng(23)
    ql = (ot.jpeg_qtable(60, 0) * rng.uniform(0.7, 1.3, (8, 8))).astype(np.float32)
    qc = (ot.jpeg_qtable(60, 1) * rng.uniform(0.7, 1.3, (8, 8))).astype(np.float32)
    return np.stack([ql, qc, qc])


# name -> shape, tables, image (util.natural_images(seed) or flat white) and grad_tol, the gradient tolerance relative to max|ref|.
# The yardstick is the oracle's own float32-vs-float64 difference (reference_arrays at both dtypes, CPU only; the figures are in
# DESIGN.md 4k): the kernel's float32 transform differs from torch's in summation order only, so it gets 4 x that floor.
#   - first, second, fourth and fifth case: 1e-3 at q60 and 1.2e-2 at q95, 4 x the floors 2.3e-4 / 2.9e-3.  The floor moves by 10 x
#     with the image (25-wide kernel, float32 z of up to several hundred), so the seeds are ones at which the oracle's floor is
#     inside those figures: 1.6e-4, 1.8e-4, 1.8e-4 and 2.7e-3 here.
#   - (5,24,64): floor 3.3e-4 -> 1.32e-3.  Tables of ones: |z| up to ~1000, floor 8.5e-3 -> 3.4e-2.  Non-integer tables: floor
#     1.6e-4, inside the q60 figure.  Flat white: the reference is below 1e-17 everywhere, GRAD_ATOL decides.
# The entropy itself differs by at most 3.1e-7 between the two oracle runs in every case: VALUE_TOL serves all of them.
CASES = {
    'one-block-q60': dict(shape=(1, 8, 8), q='q60', image='natural', grad_tol=1e-3),
    'ragged-strip-q60': dict(shape=(2, 24, 72), q='q60', image='natural', seed=5, grad_tol=1e-3),
    'part-filled-group-q60': dict(shape=(5, 24, 64), q='q60', image='natural', grad_tol=1.32e-3),
    'q60': dict(shape=(3, 32, 48), q='q60', image='natural', grad_tol=1e-3),
    'q95-full-loop': dict(shape=(3, 32, 48), q='q95', image='natural', grad_tol=1.2e-2),
    'ones': dict(shape=(3, 32, 48), q='ones', image='natural', grad_tol=3.4e-2),
    'ones-flat-white': dict(shape=(3, 32, 48), q='ones', image='white', grad_tol=1e-3),
    'non-integer-tables': dict(shape=(3, 32, 48), q='nonint', image='natural', grad_tol=1e-3),
}


def case_inputs(name):
    c = CASES[name]
    n, h, w = c['shape']
    x = np.ones((n, h, w, 3), np.float32) if c['image'] == 'white' else natural_images(n, h, w, seed=c.get('seed', 1))
    q = {'q60': lambda: ijg(60), 'q95': lambda: ijg(95), 'ones': lambda: np.ones((3, 8, 8), np.float32),
         'nonint': noninteger_tables}[c['q']]()
    return x, q


def entropy_of(e):
    """oracle/tfops.py entropy of a tensor of quantised values, as it stands."""
    return T.entropy(e.reshape(-1), torch.from_numpy(CODEBOOK), V, GAMMA)[0]


def reference_arrays(x, q, mode, dtype=torch.float64, grad=True):
    """(H, dH/dx, dH/dq (2,8,8)) of the reference at `dtype` for the transform (the estimator is float64 either way)."""
    xt = torch.tensor(np.asarray(x), dtype=dtype).requires_grad_(grad)
    qt = torch.tensor(np.asarray(q), dtype=dtype).requires_grad_(grad)
    e = odj.djpeg_torch(xt, mode=mode, q=qt)[2]
    H = entropy_of(e)
    if not grad:
        return float(H), None, None
    H.backward()
    gq = qt.grad.numpy().astype(np.float64)
    return float(H.detach()), xt.grad.numpy().astype(np.float64), np.stack([gq[0], gq[1] + gq[2]])


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """The float64 reference of a case, computed once and shared by the tests that need it (treat as read-only)."""
    x, q = case_inputs(name)
    out = reference_arrays(x, q, mode)
    for a in out[1:]:
        a.setflags(write=False)
    return out


# ---- the five-centre window (latent.hip above t_weight; csrc/djpeg_entropy.hip hist_add / entropy_dde) --------------------------
def weight(u, c):
    t = GAMMA * (np.asarray(u, np.float64)[..., None] - c)
    return (1.0 + t * t / V) ** (-(V + 1.0) / 2.0) + EPS


def full_weights(u):
    """Normalised weights (len(u), 512) over every centre."""
    w = weight(u, CODEBOOK)
    return w / w.sum(axis=1, keepdims=True)


def window_weights(u):
    """The kernel's rule: inside [LO, HI] the five centres around rint(u) (fewer at the ends of the code book), outside all 512."""
    u = np.asarray(u, np.float64)
    out = np.zeros((u.size, CODEBOOK.size))
    inside = (u >= LO) & (u <= HI)
    out[~inside] = full_weights(u[~inside])
    k0 = np.clip(np.rint(u[inside]).astype(np.int64) + 255, 0, 511)          # np.rint: half to even, like rintf
    k = k0[:, None] + np.arange(-2, 3)[None, :]
    ok = (k >= 0) & (k <= 511)
    kc = np.clip(k, 0, 511)
    w = np.where(ok, (1.0 + (GAMMA * (u[inside][:, None] - CODEBOOK[kc])) ** 2 / V) ** (-(V + 1.0) / 2.0) + EPS, 0.0)
    w = w / w.sum(axis=1, keepdims=True)
    rows = np.nonzero(inside)[0]
    for j in range(5):
        np.add.at(out, (rows[ok[:, j]], kc[ok[:, j], j]), w[ok[:, j], j])
    return out
