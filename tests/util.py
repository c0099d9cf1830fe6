"""Shared helpers for the parity tests (oracle on CPU float64 vs HIP kernels on the GPU)."""
import numpy as np
import torch


def natural_images(n, h, w, seed=0):
    """Natural-image-like synthetic RGB in [0,1]: low-pass blocks + ramp + noise, quantised to k/255."""
    rng = np.random.default_rng(seed)
    base = rng.random((n, h // 8 + 1, w // 8 + 1, 3))
    img = np.kron(base, np.ones((1, 8, 8, 1)))[:, :h, :w, :]
    ramp = np.linspace(0, 1, w)[None, None, :, None]
    img = 0.7 * img + 0.3 * ramp + rng.normal(0, 0.03, size=(n, h, w, 3))
    return (np.round(np.clip(img, 0, 1) * 255) / 255).astype(np.float32)


def bayer_from_rgb(rgb):
    """Position-ordered Bayer stack (N,h/2,w/2,4) of an RGB batch on a GBRG mosaic: planes taken at (0,0), (0,1), (1,0), (1,1)
    = G, B, R, G.  A synthetic RAW input for the learned pipelines (which do not care about the plane order); the parity
    tolerances of the workflow tests were tuned on it.  The reference's own order is stack_bayer() below."""
    g1 = rgb[:, 0::2, 0::2, 1]
    b = rgb[:, 0::2, 1::2, 2]
    r = rgb[:, 1::2, 0::2, 0]
    g2 = rgb[:, 1::2, 1::2, 1]
    return np.stack([g1, b, r, g2], axis=-1).astype(np.float32)


def stack_bayer(rgb):
    """RGGB-ordered stack of a GBRG mosaic like the reference's helpers/raw.py:204-225 `stack_bayer(image, 'GBRG')`: planes
    (R, G1, G2, B) taken at (1,0), (0,0), (1,1), (0,1) - what upsampling_kernel('gbrg') puts back in place."""
    return np.stack([rgb[:, 1::2, 0::2, 0], rgb[:, 0::2, 0::2, 1], rgb[:, 1::2, 1::2, 1], rgb[:, 0::2, 1::2, 2]],
                    axis=-1).astype(np.float32)


def to64(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64)


def err(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0, 0.0
    d = np.abs(a - b)
    return float(d.max()), float(d.max() / (np.abs(b).max() + 1e-30))


def assert_close(a, b, atol, rtol_max=None, what=''):
    """|a-b| <= atol  OR  (optionally) max|a-b| <= rtol_max * max|b| (gradient tensors have arbitrary scale)."""
    mx, rel = err(a, b)
    ok = mx <= atol or (rtol_max is not None and rel <= rtol_max)
    assert ok, '{}: max abs err {:.3e}, rel-to-max {:.3e} (atol {}, rtol_max {})'.format(what, mx, rel, atol, rtol_max)
    return mx, rel



def scene_images(n, h, w, seed=0, device='cpu'):
    """Synthetic photographs with the statistics the channel needs to LEARN on (bench.py's trained-parity leg,
    tools/train_parity.py): smooth colour gradients + a few soft-edged occluders + band-limited texture that is mostly
    luminance (the cross-channel correlation a demosaicer exploits) + a little sensor noise, quantised to k/255.
    Generated with torch on `device` (seeded per device type: a CPU and a GPU run draw different images) -> float32 tensor
    (n, h, w, 3).  natural_images() above stays the input of the parity tests (their tolerances were tuned on it)."""
    import torch.nn.functional as F
    dev = torch.device(device)
    g = torch.Generator(device=dev).manual_seed(int(seed))
    rnd = lambda *s: torch.rand(*s, generator=g, device=dev)
    nrm = lambda *s: torch.randn(*s, generator=g, device=dev)

    def blur(x, sigma):                                  # x (n, c, h, w): separable gaussian, reflect borders
        r = int(3 * sigma + 0.5)
        k = torch.exp(-0.5 * (torch.arange(-r, r + 1, device=dev, dtype=torch.float32) / sigma) ** 2)
        k = k / k.sum()
        c = x.shape[1]
        x = F.conv2d(F.pad(x, (r, r, 0, 0), mode='reflect'), k.view(1, 1, 1, -1).repeat(c, 1, 1, 1), groups=c)
        return F.conv2d(F.pad(x, (0, 0, r, r), mode='reflect'), k.view(1, 1, -1, 1).repeat(c, 1, 1, 1), groups=c)

    img = F.interpolate(rnd(n, 3, h // 32 + 2, w // 32 + 2), scale_factor=32, mode='bilinear', align_corners=False)
    img = 0.15 + 0.7 * img[:, :, 16:16 + h, 16:16 + w]
    yy = torch.arange(h, device=dev, dtype=torch.float32).view(1, h, 1)
    xx = torch.arange(w, device=dev, dtype=torch.float32).view(1, 1, w)
    for _ in range(3):                                   # occluders: half planes and discs with ~1 px soft edges
        th = rnd(n, 1, 1) * (2 * np.pi)
        cx, cy = rnd(n, 1, 1) * w, rnd(n, 1, 1) * h
        disc = rnd(n, 1, 1) < 0.5
        rad = (0.1 + 0.3 * rnd(n, 1, 1)) * min(h, w)
        dx, dy = xx - cx, yy - cy
        dist = torch.where(disc, rad - torch.sqrt(dx * dx + dy * dy), torch.cos(th) * dx + torch.sin(th) * dy)
        mask = torch.sigmoid(dist / 0.7)
        delta = (rnd(n, 3, 1, 1) - 0.5) * 0.7
        img = img + mask[:, None] * delta
    amp = 0.02 + 0.06 * rnd(n, 1, 1, 1)
    lum = blur(nrm(n, 1, h, w), 1.2) * 3.0
    chroma = blur(nrm(n, 3, h, w), 2.0) * 5.0
    img = img + amp * lum + 0.3 * amp * chroma + 0.004 * nrm(n, 3, h, w)
    img = torch.round(img.clamp(0, 1) * 255) / 255
    return img.permute(0, 2, 3, 1).contiguous()


def bayer_from_rgb_t(rgb):
    """bayer_from_rgb() for a torch tensor (N,h,w,3) on any device."""
    return torch.stack([rgb[:, 0::2, 0::2, 1], rgb[:, 0::2, 1::2, 2], rgb[:, 1::2, 0::2, 0], rgb[:, 1::2, 1::2, 1]],
                       dim=-1).contiguous()


def free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def collect_from_workers(make_procs, n_results, timeout, attempts=3):
    """Start the processes make_procs(port, queue) returns and collect n_results answers from the queue.  A worker that dies
    without answering ends the wait at once (not after `timeout`), and - because the rendezvous port is probed, released and only
    then listened on by rank 0, so another process can take it in between - the whole group is started again on a fresh port, up to
    `attempts` times.  Returns (results, procs) with every process joined."""
    import queue
    import time
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    last = None
    for _ in range(attempts):
        q = ctx.Queue()
        procs = make_procs(ctx, free_port(), q)
        for p in procs:
            p.start()
        res, deadline = [], time.monotonic() + timeout
        while len(res) < n_results:
            try:
                res.append(q.get(timeout=1.0))
            except queue.Empty:
                if any(p.exitcode not in (None, 0) for p in procs):
                    try:                                                   # an answer put just before the exit
                        res.append(q.get(timeout=0.5))
                        continue
                    except queue.Empty:
                        break
                if time.monotonic() > deadline:
                    break
        if len(res) == n_results:
            for p in procs:
                p.join(timeout=120)
            return res, procs
        last = [p.exitcode for p in procs]
        for p in procs:                                                    # exactly the processes started here
            if p.is_alive():
                p.kill()
            p.join(timeout=30)
    raise RuntimeError('workers did not answer in {} attempt(s); exit codes of the last one: {}'.format(attempts, last))


# ----------------------------------------------------------------------------------------------------------------------
# exact-arithmetic tests (tests/test_gpu_exact.py, tests/test_exact_helpers.py): bf16 x bf16 products are exact in float32 and
# float32 sums of integers are exact in any order while the sum of the absolute terms stays below 2^24 - so on small-integer
# operands every kernel, whatever its tiling or summation order, must reproduce the float64 oracle bit for bit.
EXACT_SUM_LIMIT = float(1 << 24)
BF16_INT_LIMIT = 256.0                     # every integer of magnitude <= 256 is a bf16 value


def ternary(shape, seed, p=0.25):
    """float32 values in {-1, 0, +1}, non-zero with probability p (operands of the cases whose result is stored as bf16)."""
    rng = np.random.default_rng(seed)
    nz = rng.random(size=shape) < p
    sign = rng.integers(0, 2, size=shape) * 2 - 1
    return (nz * sign).astype(np.float32)


def small_ints(shape, seed, m=3):
    """float32 uniform integers in [-m, m] (operands of the cases whose result is stored as float32)."""
    return np.random.default_rng(seed).integers(-m, m + 1, size=shape).astype(np.float32)


def bf16_rne(a):
    """float64 array of `a` (float32) rounded to bfloat16, round-to-nearest-even (torch's conversion)."""
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32))).to(torch.bfloat16).double().numpy()


def assert_exact(got, ref64, what=''):
    """got == ref64 in every element (compared as float64); on failure: the count and the first few (index, got, want)."""
    got = np.asarray(got).astype(np.float64)
    ref64 = np.asarray(ref64, np.float64)
    assert got.shape == ref64.shape, '{}: shape {} != {}'.format(what, got.shape, ref64.shape)
    if np.array_equal(got, ref64):
        return
    bad = np.argwhere(~(got == ref64))
    first = ['{} got {!r} want {!r}'.format(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref64[tuple(i)]))
             for i in bad[:8]]
    lo, hi = bad.min(axis=0), bad.max(axis=0)
    raise AssertionError('{}: {} of {} elements differ (index box {} .. {}); first: {}'.format(
        what, len(bad), got.size, tuple(int(v) for v in lo), tuple(int(v) for v in hi), '; '.join(first)))


def assert_exact_conditions(abs_sum, ref64, stores_bf16, scale=1.0, what=''):
    """The two conditions under which a case is exact, asserted on the reference alone: (a) the same operation on the absolute
    operands (`abs_sum`, float64) stays below 2^24 (in units of `scale`, a power of two); (b) where the kernel stores bf16,
    max|ref| <= 256 * scale."""
    a = float(np.asarray(abs_sum, np.float64).max()) / scale
    assert a < EXACT_SUM_LIMIT, '{}: sum of |terms| {} reaches 2^24 - the case is not exact'.format(what, a)
    if stores_bf16:
        b = float(np.abs(np.asarray(ref64, np.float64)).max()) / scale
        assert b <= BF16_INT_LIMIT, '{}: max|ref| {} > 256 - not every value is a bf16 number'.format(what, b)


def lrelu_f32(v64, alpha=0.2):
    """LeakyReLU as the kernels compute it: ONE float32 multiply on the (exactly representable) float32 value; -> float32."""
    v = np.asarray(v64, np.float64).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.asarray(v64, np.float64)), 'pre-activation is not a float32 value'
    return np.where(v > 0, v, np.float32(alpha) * v).astype(np.float32)


def mask_f32(v64, mask, alpha=0.2):
    """v * LeakyReLU'(mask) as the kernels compute it: one float32 multiply by 1 or float32(alpha)."""
    v = np.asarray(v64, np.float64).astype(np.float32)
    return np.where(np.asarray(mask) > 0, v, np.float32(alpha) * v).astype(np.float32)


def pool_windows(act):
    """(n, h, w, c) -> (n, h/2, w/2, c, 4): the 2x2 windows in the order (0,0), (0,1), (1,0), (1,1)."""
    act = np.asarray(act)
    n, h, w, c = act.shape
    return act.reshape(n, h // 2, 2, w // 2, 2, c).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c, 4)


def first_max_pool(act, last=False):
    """(pooled, arg-max) of MaxPool2D(2) with the FIRST maximum winning a tie (np.argmax); last=True: the wrong rule, for the
    self-test of the exact tests."""
    win = pool_windows(act)
    idx = (3 - np.argmax(win[..., ::-1], axis=-1)) if last else np.argmax(win, axis=-1)
    return win.max(axis=-1), idx.astype(np.uint8)


def unpool(gp, idx):
    """Route a pooled gradient (n, h/2, w/2, c) to the arg-max position of each 2x2 window -> (n, h, w, c)."""
    gp, idx = np.asarray(gp), np.asarray(idx)
    n, hp, wp, c = gp.shape
    dz = np.zeros((n, 2 * hp, 2 * wp, c), gp.dtype)
    for pos in range(4):
        dz[:, pos >> 1::2, pos & 1::2, :] = np.where(idx == pos, gp, 0)
    return dz


# ----------------------------------------------------------------------------------------------------------------------
# exact-arithmetic tests of the image chain (tests/test_gpu_chain_exact.py, tests/test_chain_helpers.py).  The linear kernels of
# csrc/manip.hip are float32 fmaf chains: on dyadic operands - pixels k / 256, taps and CSR values m / 64, integer gradients -
# every product and every partial sum is a multiple of 2^-14, and while the sum of the absolute terms stays below 2^24 of those
# units each of them is a float32 number, so the chain reproduces the float64 reference bit for bit in any order.
CHAIN_SCALE = 2.0 ** -14
PIXEL_GRID, TAP_GRID = 2.0 ** -8, 2.0 ** -6


def dyadic_pixels(shape, seed, kmax=256):
    """float32 pixels k / 256, k uniform in [0, kmax] (kmax = 256: the whole of [0, 1], both ends included)."""
    return (np.random.default_rng(seed).integers(0, kmax + 1, size=shape) * PIXEL_GRID).astype(np.float32)


def dyadic_taps(k, seed, total=None):
    """(k, k) float32 taps m / 64, the k * k integers m ALL DISTINCT (no flip, transposition or swap of two taps is invisible)
    and about a quarter of them negative; total (a multiple of 1/64): the exact sum of the taps."""
    rng = np.random.default_rng(seed)
    kk = k * k
    if kk == 1:
        return np.full((1, 1), 40 * TAP_GRID if total is None else total, np.float32)
    lo = -((kk + 1) // 3) - 2
    pool = np.arange(lo, lo + kk + max(8, kk // 3))
    for _ in range(10000):
        m = rng.permutation(pool)[:kk]
        if total is None:
            break
        last = int(round(total * 64)) - int(m[:-1].sum())
        if abs(last) <= 2 * len(pool) and last not in m[:-1]:
            m[-1] = last
            break
    else:
        raise ValueError('no distinct taps with the sum {}'.format(total))
    assert len(set(m.tolist())) == kk and (m < 0).any() and (total is None or m.sum() == round(total * 64))
    return (m.reshape(k, k) * TAP_GRID).astype(np.float32)


def assert_dyadic_conditions(abs_sum, ref64, operands=(), scale=CHAIN_SCALE, what=''):
    """The conditions under which a float32 chain is exact, asserted on the reference alone: every operand (array, grid) lies on
    its grid, the float64 reference lies on the grid `scale` (the product of the operands' grids, a power of two), and the same
    operation on the absolute operands (`abs_sum`) stays below 2^24 in units of `scale`."""
    for i, (a, grid) in enumerate(operands):
        q = np.asarray(a, np.float64) / grid
        assert np.array_equal(q, np.rint(q)), '{}: operand {} is not a multiple of {} - the case is not exact'.format(what, i, grid)
    q = np.asarray(ref64, np.float64) / scale
    assert np.array_equal(q, np.rint(q)), '{}: the reference is not a multiple of {} - the case is not exact'.format(what, scale)
    assert_exact_conditions(abs_sum, ref64, False, scale=scale, what=what)


def depthwise_filter(x, taps, pad_mode, dy=None, keep=None, dtype=torch.float64):
    """The per-channel k x k filter over the mirrored image as the oracle states it (oracle.tfops.pad2d + a VALID conv2d with a
    diagonal filter), before any clip: -> pre (numpy, `dtype`); with dy also the input gradient of sum(pre * dy * keep) by
    autograd (keep: 0 / 1 per element, the clip mask; None = all pass): -> (pre, dx)."""
    from oracle import tfops as T
    taps = np.asarray(taps)
    k, c = taps.shape[0], np.asarray(x).shape[3]
    gf = torch.zeros((k, k, c, c), dtype=dtype)
    for ch in range(c):
        gf[:, :, ch, ch] = torch.tensor(taps, dtype=dtype)
    xt = torch.tensor(np.asarray(x), dtype=dtype).requires_grad_(dy is not None)
    pre = T.conv2d(T.pad2d(xt, k // 2, pad_mode), gf, None, 1, 'VALID')
    if dy is None:
        return pre.numpy()
    wgt = torch.tensor(np.asarray(dy), dtype=dtype)
    if keep is not None:
        wgt = wgt * torch.tensor(np.asarray(keep), dtype=dtype)
    (pre * wgt).sum().backward()
    return pre.detach().numpy(), xt.grad.numpy()


def clip_bits(pre):
    """(n, h, w, 3) pre-clip values -> (n, h, w) uint8, bit c set where channel c passes the clip: 0 <= v <= 1, both ends
    INCLUDED (tf.clip_by_value passes the gradient on the closed interval)."""
    pre = np.asarray(pre)
    keep = (pre >= 0) & (pre <= 1)
    return (keep[..., 0] * 1 + keep[..., 1] * 2 + keep[..., 2] * 4).astype(np.uint8)


def bits_to_keep(bits):
    """(n, h, w) mask bytes -> (n, h, w, 3) float64 0 / 1."""
    bits = np.asarray(bits)
    return np.stack([(bits >> c) & 1 for c in range(3)], axis=-1).astype(np.float64)


def quantised_images(n, h, w, seed, levels=16):
    """natural_images() quantised to `levels` values j / (levels - 1): ties in nearly every window, like real k / 255 images."""
    side = max(h, w, 8)
    x = natural_images(n, side, side, seed)[:, :h, :w]
    return (np.round(x * (levels - 1)) / (levels - 1)).astype(np.float32)


def median_select(x, k, last=False):
    """(y, sel) of the k x k median as tf.nn.top_k orders it: the element of rank (k * k + 1) // 2 - 1 in STABLE DESCENDING order
    of the REFLECT-padded row-major window (among equal values the lower window index first).  last=True: among equal values
    the higher index first - the wrong rule, for the self-test."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    r, area = k // 2, k * k
    xp = np.pad(x, ((0, 0), (r, r), (r, r), (0, 0)), mode='reflect') if r else x
    win = np.stack([xp[:, a:a + h, b:b + w, :] for a in range(k) for b in range(k)], axis=-1)
    if last:
        sel = (area - 1 - np.argsort(-win[..., ::-1], axis=-1, kind='stable'))[..., (area + 1) // 2 - 1]
    else:
        sel = np.argsort(-win, axis=-1, kind='stable')[..., (area + 1) // 2 - 1]
    y = np.take_along_axis(win, sel[..., None], axis=-1)[..., 0]
    return y, sel.astype(np.uint8)


def median_scatter(dy, sel, k):
    """Route dy to the selected element of each window (REFLECT-mapped back onto the image) -> dx, float64."""
    dy, sel = np.asarray(dy, np.float64), np.asarray(sel).astype(np.int64)
    n, h, w, c = dy.shape
    r = k // 2

    def mirror(i, size):
        i = np.where(i < 0, -i, i)
        return np.where(i >= size, 2 * (size - 1) - i, i)

    ni, yi, xi, ci = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(c), indexing='ij')
    yy, xx = mirror(yi + sel // k - r, h), mirror(xi + sel % k - r, w)
    dx = np.zeros_like(dy)
    np.add.at(dx, (ni, yy, xx, ci), dy)
    return dx


def csr_of(dense):
    """(rowptr, col, val) of a dense (out, in) operator, zeros dropped, columns ascending - numpy int32 / int32 / float32."""
    dense = np.asarray(dense)
    rowptr, col, val = [0], [], []
    for row in dense:
        nz = np.nonzero(row)[0]
        col.extend(nz.tolist())
        val.extend(row[nz].tolist())
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float32)


def redraw_near_half(x, value_of, seed, width=1e-3, lo=0.05, hi=0.95):
    """Redraw (float64 arithmetic, CPU) every element of the float32 array x whose reference 255 * value_of(x) lies within
    `width` of a half-integer, until none does: a float32 evaluation of 255 * v (error < 1e-4) then rounds as float64 does."""
    rng = np.random.default_rng(seed)
    x = np.array(x, np.float32)
    for _ in range(100):
        v = 255.0 * np.asarray(value_of(x.astype(np.float64)), np.float64)
        bad = np.abs(v - np.floor(v) - 0.5) <= width
        if not bad.any():
            return x
        x[bad] = (lo + (hi - lo) * rng.random(int(bad.sum()))).astype(np.float32)
    raise AssertionError('could not move every element away from the rounding ties')


# ----------------------------------------------------------------------------------------------------------------------
# exact-arithmetic tests of the tail of the training step (tests/test_gpu_tail_exact.py, tests/tail_cases.py,
# tests/test_tail_helpers.py): losses, sums, FAN head, Adam, latent.
F32_UNIT_ROUNDOFF = 2.0 ** -24
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def odd_part(n):
    """n / (the largest power of two dividing n)."""
    n = int(n)
    assert n > 0
    return n // (n & -n)


def is_f32(a64):
    """Every element of the float64 array is a float32 number (nothing would round on a float32 store)."""
    a64 = np.asarray(a64, np.float64)
    return np.array_equal(a64.astype(np.float32).astype(np.float64), a64)


def assert_no_denormals(*arrays, what=''):
    """No operand or intermediate may be a float32 denormal: every non-zero magnitude is at least 2^-126."""
    for i, a in enumerate(arrays):
        a = np.abs(np.asarray(a, np.float64))
        nz = a[a != 0]
        assert nz.size == 0 or float(nz.min()) >= F32_MIN_NORMAL, '{}: array {} holds a float32 denormal ({})'.format(what, i, nz.min())


def pixel_pairs(shape, seed, j=None, jmax=127):
    """(a, b, j): float32 pixels a = ka / 256, b = kb / 256 in [0, 1] with ka - kb = j, |j| <= jmax (drawn uniformly unless
    given): a - b = j / 256, 255 (a - b) and 255 a - 255 b are exact in float32."""
    rng = np.random.default_rng(seed)
    if j is None:
        j = rng.integers(-jmax, jmax + 1, size=shape)
    j = np.asarray(j, np.int64)
    assert np.abs(j).max(initial=0) <= 127
    lo, hi = np.maximum(0, -j), np.minimum(256, 256 - j)                   # kb in [lo, hi] keeps ka = kb + j inside [0, 256]
    kb = lo + np.floor(rng.random(size=j.shape) * (hi - lo + 1)).astype(np.int64)
    ka = kb + j
    assert ka.min(initial=0) >= 0 and ka.max(initial=0) <= 256 and kb.min(initial=0) >= 0 and kb.max(initial=0) <= 256
    return (ka * PIXEL_GRID).astype(np.float32), (kb * PIXEL_GRID).astype(np.float32), j


def depth_to_space2(q):
    """(n, h, w, 4 c) -> (n, 2 h, 2 w, c), the inverse of oracle.tfops.space_to_depth(x, 2): channel (2 pr + pc) c + ch of block
    (y, x) is pixel (2 y + pr, 2 x + pc), channel ch."""
    q = np.asarray(q)
    n, h, w, c4 = q.shape
    c = c4 // 4
    return q.reshape(n, h, w, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, 2 * h, 2 * w, c)


def space_to_depth2(x):
    x = np.asarray(x)
    n, h2, w2, c = x.shape
    return x.reshape(n, h2 // 2, 2, w2 // 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h2 // 2, w2 // 2, 4 * c)


def pack_bits(bits, axis_len=32):
    """(..., 32) booleans -> (...) int32 words, bit j of a word = element j."""
    bits = np.asarray(bits).astype(np.uint64)
    assert bits.shape[-1] == axis_len == 32
    return (bits << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32).view(np.int32)


# ----------------------------------------------------------------------------------------------------------------------
# exact-arithmetic tests of the glue kernels (tests/test_gpu_glue_exact.py, tests/glue_cases.py, tests/test_glue_helpers.py):
# pooling, layout, element-wise streams, SSIM family.  Routing and permutation kernels get operands whose elements differ from
# one another, so that no transposition, phase swap or lane swap is invisible.
def distinct_ints(shape, seed, lo=1):
    """float32 integers lo, lo + 1, ... in a random order, every element different (the count must stay below 2^24)."""
    count = int(np.prod(shape))
    assert abs(lo) + count < (1 << 24)
    return (np.random.default_rng(seed).permutation(count) + lo).reshape(shape).astype(np.float32)


def distinct_bf16(shape, seed, period=16001):
    """float32 array of bfloat16 NUMBERS, normal and finite, of both signs: bit patterns 0x3800 + (a random permutation of the
    indices modulo `period`), so all elements differ while the count stays within `period`, and any two elements less than
    `period` apart in the drawing order differ beyond it."""
    count = int(np.prod(shape))
    order = np.random.default_rng(seed).permutation(count) if count <= (1 << 22) else np.arange(count)
    bits = (0x3800 + order % period).astype(np.uint32)
    bits |= np.where(order % 3 == 0, 0x8000, 0).astype(np.uint32)
    v = (bits << 16).view(np.float32).reshape(shape)
    assert np.isfinite(v).all() and np.abs(v).min() >= F32_MIN_NORMAL
    return v


def lane_complete_argmax(shape, seed):
    """(n, ho, wo, c) random arg-max bytes 0..3 in which every channel lane of every 8-channel granule holds all four values
    (the first four pixels of the batch are planted: pixel p, channel ch gets (p + ch + ch // 4) % 4)."""
    n, ho, wo, c = shape
    idx = np.random.default_rng(seed).integers(0, 4, size=shape).astype(np.uint8)
    flat = idx.reshape(n * ho * wo, c)
    assert flat.shape[0] >= 4, 'four pixels are needed to hold all four values in a lane'
    ch = np.arange(c)
    for p in range(4):
        flat[p] = (p + ch + ch // 4) % 4
    idx = flat.reshape(shape)
    for lane in range(c):
        assert set(np.unique(idx[..., lane]).tolist()) == {0, 1, 2, 3}
    return idx
