"""
The dJPEG rate term (csrc/djpeg_entropy.hip) held to references that start from the kernels' own z: cases, inputs,
references, floors and tolerances in tests/djpeg_rate_cases.py, their conditions proved on the CPU by tests/test_djpeg_rate_cases.py.
tests/test_gpu_djpeg_entropy.py stays the end-to-end check from x.

  * g_k = dH / d mean_k, the float64 the backward pass reads (the first 512 float64 of the workspace after _fwd): 1e-10 of max|g_ref|
    where e is exact (round, soft, identity), 4 F_e under sin / harmonic;
  * H: 2 ulp of float32, plus 4 F_e under the smooth modes;
  * gx and dq: 4 (F_t + F_e) + A of max|ref| per run - 1e-7 .. 1.6e-2 where the end-to-end tolerances are 1e-3 .. 3.4e-2;
  * exactly: no gradient at all under round, accumulate == old + written bit for bit, dq = None changes nothing at integer tables.

Every run is all five rounding templates' business: round and identity are launched here for the first time.  Every buffer sits
between guard bytes, and a gx that is written, not accumulated, starts as NaN.
"""
import numpy as np
import pytest
import torch

import djpeg_rate_cases as R

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    return torch.device('cuda', 0)


def g32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev).contiguous()


class Guarded(object):
    """`nbytes` of device memory between two runs of 0xa5 bytes (the pattern of tests/test_gpu_djpeg_entropy.py)."""

    def __init__(self, nbytes, dev, fill=None):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), 0xa5, dtype=torch.uint8, device=dev)
        self.bytes = self.buf[GUARD:GUARD + self.n]
        if fill is not None:
            self.bytes.copy_(fill.contiguous().view(torch.uint8).reshape(-1))

    def f32(self, *shape):
        return self.bytes.view(torch.float32).view(*shape)

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:GUARD] == 0xa5).all()) and bool((b[GUARD + self.n:] == 0xa5).all())


class Launch(object):
    """One _fwd of a run inside guard bytes; bwd() may follow any number of times."""

    def __init__(self, dev, case, kind, tab, mode):
        from neural_imaging_amd import _lib, ops
        self.dev, self.mode, self.ops = dev, mode, ops
        x = R.inputs(case, kind)
        self.shape = x.shape
        n, h, w, _ = x.shape
        self.x, self.q = Guarded(x.size * 4, dev, g32(x, dev)), Guarded(192 * 4, dev, g32(R.table(tab), dev))
        self.ws = Guarded(_lib.load().nimg_djpeg_entropy_workspace_bytes(n, h, w), dev)
        self.ent = Guarded(4, dev)
        self.buffers = [('x', self.x), ('q', self.q), ('workspace', self.ws), ('entropy', self.ent)]
        ops.djpeg_entropy_fwd(self.x.f32(*x.shape), self.q.f32(3, 8, 8), mode, ws=self.ws.bytes, out=self.ent.f32(1))
        torch.cuda.synchronize(dev)
        self.H = float(self.ent.f32(1)[0])
        self.g = self.ws.bytes[:512 * 8].view(torch.float64).cpu().numpy().copy()      # the layout comment of the kernel, nimg.h

    def bwd(self, gx0=None, dq0=None, want_dq=True, coef=1.0):
        """gx and dq as float32 device tensors.  gx0 / dq0: accumulate onto these contents; otherwise gx starts as NaN and dq as
        0xa5 bytes, and both are overwritten."""
        nan = torch.full(self.shape, float('nan'), dtype=torch.float32, device=self.dev)
        gx = Guarded(nan.numel() * 4, self.dev, nan if gx0 is None else gx0)
        dq = Guarded(128 * 4, self.dev, dq0) if want_dq else None
        self.ops.djpeg_entropy_bwd(self.x.f32(*self.shape), self.q.f32(3, 8, 8), self.ws.bytes, coef, self.mode,
                                   out=gx.f32(*self.shape), accumulate=gx0 is not None,
                                   dq=dq.f32(2, 8, 8) if want_dq else None, accumulate_dq=dq0 is not None)
        torch.cuda.synchronize(self.dev)
        for what, b in self.buffers + [('gx', gx)] + ([('dq', dq)] if want_dq else []):
            assert b.intact(), '{}: guard bytes overwritten'.format(what)
        return gx.f32(*self.shape).clone(), (dq.f32(2, 8, 8).clone() if want_dq else None)


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def check(what, got, ref, tol, atol=0.0, top=None):
    """max|got - ref| <= tol * max|ref| + atol (top: the max|ref| to go by, where ref is a part of a larger reference); the figure
    is printed before it is asserted."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all(), '{}: not finite (an element was left unwritten?)'.format(what)
    top = np.abs(ref).max() if top is None else top
    diff = np.abs(got - ref).max()
    print('{}: max|diff| {:.3e} = {:.3e} of max|ref| {:.3e}; tolerance {:.3e}'.format(what, diff, diff / top if top else 0.0, top, tol))
    assert diff <= tol * top + atol, '{}: {:.3e} of max|ref| > {:.3e}'.format(what, diff / top if top else np.inf, tol)


@pytest.mark.parametrize('case,kind,tab,mode', R.RUNS, ids=R.RUN_IDS)
def test_value_and_gradients(dev, case, kind, tab, mode):
    ref = R.reference(case, kind, tab, mode)
    run = Launch(dev, case, kind, tab, mode)
    name = '-'.join((case, kind, tab, mode))
    print(R.describe(case, kind, tab, mode, ref))
    check(name + ' g', run.g, ref['g'], ref['tol_g'])
    # the clip mask of the histogram, two-sided: g is exactly 0 under the clip and nowhere else
    assert np.array_equal(run.g == 0, ref['hm'] < R.CLIP)
    print('{} H: {:.7f}, reference {:.7f}, |diff| {:.3e} = {:.2f} ulp; tolerance {:.3e}'.format(
        name, run.H, ref['H'], abs(run.H - ref['H']), abs(run.H - ref['H']) / R.ulp32(ref['H']), ref['tol_H']))
    assert abs(run.H - ref['H']) <= ref['tol_H']
    gx, dq = run.bwd()
    gx, dq = gx.cpu().numpy(), dq.cpu().numpy()
    _, index = R.batch(case, kind)
    gx_ref = ref['gx'][index]
    if mode == 'round':
        # G_ZERO: no gradient at all, also under tables of ones, where `soft` carries one
        assert not gx_ref.any() and not ref['dq'].any()
        assert np.isfinite(gx).all() and (gx == 0).all() and (dq == 0).all()
    else:
        check(name + ' gx', gx, gx_ref, ref['tol_gx'], R.TINY)
        check(name + ' dq', dq, ref['dq'], ref['tol_dq'], R.TINY)
    if case == 'grid-cap':
        # tasks 4096 .. 4111, the second iteration of the 16 waves of workgroups 0 .. 3: images 2048 .. 2055, on their own
        first = 4 * R.grid_of(R.CASES[case]) // 2
        assert first == 2048
        if mode == 'round':
            assert (gx[first:] == 0).all()
        else:
            top = np.abs(gx_ref).max()
            check(name + ' gx, first iteration (images 0 .. 2047)', gx[:first], gx_ref[:first], ref['tol_gx'], R.TINY, top)
            check(name + ' gx, second iteration (images 2048 .. 2055)', gx[first:], gx_ref[first:], ref['tol_gx'], R.TINY, top)
            assert np.abs(gx_ref[first:]).max() > 0.1 * top


EXACT_RUNS = [('three-strips', 'saturated', 'q50', 'sin'), ('seg-33', 'noise', 'frac', 'harmonic'),
              ('codebook-sweep', 'sweep', 'sweep-int', 'identity'), ('grid-cap', 'saturated', 'q50', 'sin'),
              ('full+ragged', 'noise', 'ones', 'soft')]


@pytest.mark.parametrize('case,kind,tab,mode', EXACT_RUNS, ids=['-'.join(r) for r in EXACT_RUNS])
def test_accumulate_is_old_plus_written_bit_for_bit(dev, case, kind, tab, mode):
    """One _fwd, then a written and an accumulated backward pass.  The backward kernel has no atomics and reads its old gx once, so
    gx_acc == gx0 + gx_written in float32; launch_reduce2 sums the 4 x grid partial rows in its fixed order and adds the old dq
    LAST (reduce_slabs: r += old), so dq_acc == dq_written + dq0 in float32 as well."""
    run = Launch(dev, case, kind, tab, mode)
    gx_w, dq_w = run.bwd()
    assert float(gx_w.abs().max()) > 0 and float(dq_w.abs().max()) > 0
    rng = np.random.default_rng(7)
    gx0 = g32(rng.normal(0, float(gx_w.abs().max()), run.shape), run.dev)
    dq0 = g32(rng.normal(0, float(dq_w.abs().max()), (2, 8, 8)), run.dev)
    gx_a, dq_a = run.bwd(gx0=gx0, dq0=dq0)
    assert same_bits(gx_a, gx0 + gx_w)
    assert same_bits(dq_a, dq_w + dq0)
    # each flag on its own
    gx_b, dq_b = run.bwd(gx0=gx0)
    assert same_bits(gx_b, gx_a) and same_bits(dq_b, dq_w)
    gx_c, dq_c = run.bwd(dq0=dq0)
    assert same_bits(gx_c, gx_w) and same_bits(dq_c, dq_a)
    # dq = None: the same image gradient.  Without dq integer tables take the Markstein division, the exact one there (it differs
    # in the sign of a zero z, which neither e, the surrogate nor G sees); non-integer tables divide by IEEE either way.
    gx_n, _ = run.bwd(want_dq=False)
    assert same_bits(gx_n, gx_w)


@pytest.mark.parametrize('case,kind,tab', [r[:3] for r in EXACT_RUNS], ids=['-'.join(r[:3]) for r in EXACT_RUNS])
def test_round_gives_the_old_contents_back(dev, case, kind, tab):
    run = Launch(dev, case, kind, tab, 'round')
    rng = np.random.default_rng(8)
    gx0, dq0 = g32(rng.normal(0, 1, run.shape), run.dev), g32(rng.normal(0, 1, (2, 8, 8)), run.dev)
    gx_a, dq_a = run.bwd(gx0=gx0, dq0=dq0, coef=3.0)
    assert same_bits(gx_a, gx0) and same_bits(dq_a, dq0)
    gx_n, _ = run.bwd(gx0=gx0, want_dq=False)
    assert same_bits(gx_n, gx0)
