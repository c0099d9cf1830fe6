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
