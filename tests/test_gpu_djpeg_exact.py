"""
Exact, every-route tests of the differentiable JPEG kernels (csrc/djpeg.hip) and of the clip mask of the sub-sampled ones
(csrc/djpeg_sub.hip).  Cases, inputs and references: tests/djpeg_cases.py; the conditions they have to meet are proved on the CPU
by tests/test_djpeg_cases.py and asserted again here where a test relies on them.

A wave task is one 8-row strip of up to 64 pixels, four tasks per workgroup.  The six shapes are the smallest with idle waves
(`t.valid == false`: 3, 2 and 1 of them), a ragged strip alone, a full strip before a ragged one, three strips per row, a task
count that is no multiple of four, and - the control - neither.  The `saturated` input clips a quarter of the pre-clip values, so
the ZERO bits of the clip mask are checked, which the older tests (one-sided: "inside => bit set") cannot see.

1. hard rounding (test_forward_hard): idx, xdq, y and the mask BIT FOR BIT against the C oracle in the canonical float32 order, on
   the integer route (Markstein division: IJG q10 / q50 / q95, all-ones) and the IEEE-division route (`frac`, and `last`: one
   non-integer at the last staged entry); `round` and `soft` give the same bits, and so does every combination of optional outputs.
2. smooth modes (test_forward_smooth): y at 1e-4 and the mask, both ways, against float64.
3. backward (test_backward): gx and the table gradient against autograd of the float64 restatement at a given mask - the oracle's
   (a quarter of its bits clear), none, and a pattern that tells the three bits and the eight byte positions of a packed mask row
   apart; accumulation, sentinels, guard bands, repeatability, an image alone against the image in its batch.
4. the sub-sampled kernels' own forward mask, both ways, and their backward pass fed with it.

Kernel instantiation reached by each test id (read off nimg_djpeg_fwd and launch_bwd in csrc/djpeg.hip; the division route is
chosen per launch by stage_tables: integer tables in 1 .. 255 take div_q<false>, any other entry div_q<true>; the backward kernels
with the table gradient always divide):

  djpeg_fwd_kernel<Q_RINT>       integer route   forward_hard[*-q10|q50|q95|ones], optional_outputs[*-q50], guard_bands[*-q50], repeats
                                 IEEE route      forward_hard[*-frac|last], optional_outputs[*-frac], guard_bands[*-frac]
  djpeg_fwd_kernel<Q_SIN>        both routes     forward_smooth[*-q50-sin] / [*-frac-sin]
  djpeg_fwd_kernel<Q_HARMONIC>   both routes     forward_smooth[*-q50-harmonic] / [*-frac-harmonic]
  djpeg_fwd_kernel<Q_IDENTITY>   both routes     forward_smooth[*-q50-identity] / [*-frac-identity]
  djpeg_bwd_kernel<ROUND, false>     backward[*-round-*]      (integer route at q50, IEEE route at frac)
  djpeg_bwd_kernel<SOFT, false>      backward[*-soft-*] AND backward[*-sin-*]: without the table gradient launch_bwd sends SIN to the
                                     SOFT kernel (the same gradient of x); guard_bands, repeats, image_alone
  djpeg_bwd_kernel<HARMONIC, false>  backward[*-harmonic-*]
  djpeg_bwd_kernel<IDENTITY, false>  backward[*-identity-*]
  djpeg_bwd_kernel<ROUND, true>      backward[*-round-*] (dq = sum of rint(z) d loss / d Xd: the only gradient of `round`)
  djpeg_bwd_kernel<SOFT, true>       backward[*-soft-*], dq_accumulate, guard_bands, repeats
  djpeg_bwd_kernel<SIN, true>        backward[*-sin-*] (its own kernel: quantise<Q_SIN> enters the table gradient)
  djpeg_bwd_kernel<HARMONIC, true>   backward[*-harmonic-*]
  djpeg_bwd_kernel<IDENTITY, true>   backward[*-identity-*] (the table gradient cancels: exactly zero)
  djpeg_sub.hip forward and backward, 4:2:0 and 4:2:2, every mode: sub_forward_mask, sub_backward_with_the_kernels_mask
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import djpeg_cases as C
from util import assert_close, bits_to_keep

pytestmark = pytest.mark.gpu

ATOL = 1e-4          # tests/test_gpu_ops.py
GRTOL = 1e-4
GUARD = 4096         # bytes on either side of every output
GUARD_CASES = ['full+ragged', 'three-strips', 'one-block']
ERRORS = {}          # (mode, 'gx' | 'dq', route) -> largest error seen, as a fraction of max|ref|


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    t0 = time.monotonic()
    yield torch.device('cuda', 0)
    for key in sorted(ERRORS):
        print('djpeg exact: largest error / max|ref| of {} {} ({}): {:.2e}'.format(*key, ERRORS[key]))
    print('djpeg exact: module wall time {:.1f} s'.format(time.monotonic() - t0))        # (shown with pytest -s)


def g(a, dev, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(dev).contiguous()          # (np.array: always a copy)


def host(t):
    return None if t is None else t.cpu().numpy()


def forward(dev, x, q, mode, **want):
    from neural_imaging_amd import ops
    want = dict(dict(want_mask=True, want_idx=True, want_xdq=True), **want)
    y, mask, idx, xdq = ops.djpeg_fwd(g(x, dev), g(q, dev), mode, **want)
    return dict(y=host(y), mask=host(mask), idx=host(idx), xd=host(xdq))


def assert_same(got, want, what):
    """Equal values in every element (np.array_equal: -0 == +0, the one difference the Markstein division is allowed)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    first = ['{} got {!r} want {!r}'.format(tuple(int(v) for v in i), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:6]]
    raise AssertionError('{}: {} of {} elements differ (index box {} .. {}); first: {}'.format(
        what, len(bad), got.size, tuple(int(v) for v in bad.min(axis=0)), tuple(int(v) for v in bad.max(axis=0)), '; '.join(first)))


def assert_mask_two_sided(mask, ref_mask, leave_out, what):
    """Every bit outside `leave_out` ((n,h,w,3) booleans) equals the reference's, the clear ones included; bits 3 .. 7 are clear."""
    assert mask.max() <= 7, '{}: a mask byte above 7'.format(what)
    got, want = bits_to_keep(mask).astype(bool), bits_to_keep(ref_mask).astype(bool)
    care = ~leave_out
    wrong = (got != want) & care
    assert not wrong.any(), '{}: {} of {} compared bits differ ({} set for clear, {} clear for set)'.format(
        what, int(wrong.sum()), int(care.sum()), int((wrong & got).sum()), int((wrong & want).sum()))
    assert (~want & care).any() and (want & care).any(), what + ': the comparison saw only one kind of bit'


# ------------------------------------------------------------------------------------------------------------------------------
# 1. forward, hard rounding: bit for bit
@pytest.mark.parametrize('tab', C.TABLES)
@pytest.mark.parametrize('kind', C.INPUTS)
@pytest.mark.parametrize('case', C.CASE_IDS)
def test_forward_hard(dev, case, kind, tab):
    """Measured on the MI355X: y and the mask ARE bit-equal to the C oracle on both division routes - the kernel's Markstein / 255
    is the IEEE quotient - so the comparison is np.array_equal throughout and no bit is left out."""
    ref = C.hard_reference(case, kind, tab)
    x, q = C.images(C.CASES[case], kind), C.table(tab)
    if kind == 'saturated':
        assert C.CLIP_SHARE[0] <= C.clear_share(ref['mask']) <= C.CLIP_SHARE[1]
    outs = {mode: forward(dev, x, q, mode) for mode in C.HARD_MODES}
    for mode, out in outs.items():
        what = 'djpeg fwd {} {} {} {}: '.format(case, kind, tab, mode)
        assert_same(out['idx'], ref['idx'], what + 'idx')
        assert_same(out['xd'], ref['xd'], what + 'xdq')
        print(what + 'max|y - oracle| = {:.3e}, mask bytes differing: {}'.format(
            float(np.abs(out['y'] - ref['y']).max()), int((out['mask'] != ref['mask']).sum())))
        assert_same(out['y'], ref['y'], what + 'y')
        assert out['mask'].max() <= 7
        assert_same(out['mask'], ref['mask'], what + 'mask')
    for k in ('y', 'mask', 'idx', 'xd'):
        assert_same(outs['round'][k], outs['soft'][k], 'round against soft: ' + k)


@pytest.mark.parametrize('tab', ['q50', 'frac'])
@pytest.mark.parametrize('case', C.CASE_IDS)
def test_forward_optional_outputs(dev, case, tab):
    """`if (idx || xdq)`: none of the eight combinations of optional outputs changes a bit of y or of the outputs that are asked for."""
    x, q = C.images(C.CASES[case], 'saturated'), C.table(tab)
    for mode in ('soft', 'sin'):
        full = forward(dev, x, q, mode)
        if mode == 'soft':
            assert_same(full['y'], C.hard_reference(case, 'saturated', tab)['y'], 'y')
        for bits in range(8):
            want = dict(want_mask=bool(bits & 1), want_idx=bool(bits & 2), want_xdq=bool(bits & 4))
            out = forward(dev, x, q, mode, **want)
            assert_same(out['y'], full['y'], 'y with {}'.format(want))
            for k, asked in (('mask', want['want_mask']), ('idx', want['want_idx']), ('xd', want['want_xdq'])):
                if asked:
                    assert_same(out[k], full[k], '{} with {}'.format(k, want))
                else:
                    assert out[k] is None


# ------------------------------------------------------------------------------------------------------------------------------
# 2. forward, smooth modes
@pytest.mark.parametrize('mode', C.SMOOTH_MODES)
@pytest.mark.parametrize('tab', ['q50', 'frac'])
@pytest.mark.parametrize('kind', C.SMOOTH_INPUTS)
@pytest.mark.parametrize('case', C.CASE_IDS)
def test_forward_smooth(dev, case, kind, tab, mode):
    ref = C.smooth_reference(case, kind, tab, mode)
    out = forward(dev, C.images(C.CASES[case], kind), C.table(tab), mode, want_idx=False, want_xdq=False)
    assert_close(out['y'], ref['y'], ATOL, what='djpeg fwd {} {} {} {}'.format(case, kind, tab, mode))
    edge = C.near_edge(ref['pre'], C.EDGE_SMOOTH)
    if C.edge_cap_holds(mode, kind):
        assert edge.mean() <= C.EDGE_CAP
    if kind == 'noise' and not (~bits_to_keep(ref['mask']).astype(bool) & ~edge).any():
        assert out['mask'].max() <= 7              # (a small noise image may clip nowhere: then every compared bit is set)
        assert np.array_equal(bits_to_keep(out['mask']).astype(bool) | edge, np.ones_like(edge))
        return
    assert_mask_two_sided(out['mask'], ref['mask'], edge, 'mask {} {} {} {}'.format(case, kind, tab, mode))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. backward
def backward(dev, x, gy, mask, q, mode, dq=None, accumulate=False):
    from neural_imaging_amd import ops
    gx = ops.djpeg_bwd(g(x, dev), g(gy, dev), g(mask, dev, np.uint8), g(q, dev), mode, dq=dq, accumulate=accumulate)
    return host(gx)


def note(mode, what, route, got, ref):
    scale = float(np.abs(ref).max())
    if scale > 0:
        key = (mode, what, route)
        ERRORS[key] = max(ERRORS.get(key, 0.0), float(np.abs(got - ref).max()) / scale)


@pytest.mark.parametrize('tab', ['q50', 'frac'])
@pytest.mark.parametrize('mode', C.MODES)
@pytest.mark.parametrize('case', C.CASE_IDS)
def test_backward(dev, case, mode, tab):
    """gx (both entry points) and dq against autograd of the float64 restatement without its clip, the mask given to both sides.
    dq per entry: |got - ref| <= 1e-6 + 3e-4 max|ref of its table| + allowance, the allowance being zero for the smooth modes and,
    for `round` and `soft`, what the coefficients within 1e-3 of a rounding tie could move the entry by (at most 1 % of them)."""
    shape = C.CASES[case]
    x, gy = C.images(shape, 'saturated'), C.gradient(shape)
    ql, qc = C.table_pair(tab)
    q = C.table(tab)
    oracle_mask = C.hard_reference(case, 'saturated', tab)['mask']
    assert C.CLIP_SHARE[0] <= C.clear_share(oracle_mask) <= C.CLIP_SHARE[1]
    route = 'integer tables' if C.is_integer_table(q) else 'IEEE division'
    for name, mask in (('oracle', oracle_mask), ('none', np.zeros(shape, np.uint8)), ('pattern', C.pattern_mask(shape))):
        what = 'djpeg bwd {} {} {} mask={}: '.format(case, mode, tab, name)
        ref = C.backward_reference(x, gy, ql, qc, mode, mask)
        assert ref['tie_share'] <= C.TIE_CAP
        dq_t = torch.full((2, 8, 8), float('nan'), device=dev)
        gx = backward(dev, x, gy, mask, q, mode)
        gx_dq = backward(dev, x, gy, mask, q, mode, dq=dq_t)
        dq = host(dq_t)
        if name == 'none':
            assert not ref['gx'].any() and not ref['dq'].any()
            assert not gx.any() and not gx_dq.any() and not dq.any(), what + 'a gradient where every bit is clear'
            continue
        if mode == 'round':
            assert not ref['gx'].any() and not gx.any() and not gx_dq.any(), what + 'the rounding has no gradient'
        else:
            note(mode, 'gx', route, gx, ref['gx'])
            note(mode, 'gx', 'table-gradient kernel', gx_dq, ref['gx'])
            assert_close(gx, ref['gx'], 1e-5, GRTOL * 3, what=what + 'gx')
            assert_close(gx_dq, ref['gx'], 1e-5, GRTOL * 3, what=what + 'gx of the table-gradient kernel')
        if mode == 'identity':
            assert not dq.any(), what + 'z - z * 1 is zero: the tables cancel exactly'
        for k in range(2):
            bound = 1e-6 + 3 * GRTOL * np.abs(ref['dq'][k]).max() + (ref['allow'][k] if mode in C.HARD_MODES else 0.0)
            d = np.abs(dq[k] - ref['dq'][k])
            if mode in C.SMOOTH_MODES and mode != 'identity':
                note(mode, 'dq', 'luma' if k == 0 else 'chroma', dq[k], ref['dq'][k])
            elif mode in C.HARD_MODES:           # the part of the error that no near-tie explains
                scale = float(np.abs(ref['dq'][k]).max())
                key = (mode, 'dq beyond the tie allowance', 'luma' if k == 0 else 'chroma')
                ERRORS[key] = max(ERRORS.get(key, 0.0), float(np.maximum(d - ref['allow'][k], 0).max()) / scale)
            assert (d <= bound).all(), what + 'dq[{}]: worst excess {:.3e} at {} (error {:.3e}, max|ref| {:.3e})'.format(
                k, float((d - bound).max()), np.unravel_index(np.argmax(d - bound), d.shape), float(d.max()),
                float(np.abs(ref['dq'][k]).max()))


@pytest.mark.parametrize('mode', ['soft', 'harmonic'])
@pytest.mark.parametrize('case', C.CASE_IDS)
def test_dq_accumulate(dev, case, mode):
    """accumulate = 0 overwrites whatever the buffer held (bit-equal to a fresh result); accumulate = 1 adds the same sum to the
    previous value in one float32 addition."""
    shape = C.CASES[case]
    x, gy, q = C.images(shape, 'saturated'), C.gradient(shape), C.table('frac')
    mask = C.hard_reference(case, 'saturated', 'frac')['mask']
    fresh = torch.zeros((2, 8, 8), device=dev)
    gx0 = backward(dev, x, gy, mask, q, mode, dq=fresh)
    over = torch.full((2, 8, 8), -1.25e30, device=dev)
    gx1 = backward(dev, x, gy, mask, q, mode, dq=over)
    assert torch.equal(over, fresh) and np.array_equal(gx0, gx1)
    prev = np.random.default_rng(7).uniform(-1, 1, (2, 8, 8)).astype(np.float32) * np.abs(host(fresh)).max()
    acc = g(prev, dev)
    gx2 = backward(dev, x, gy, mask, q, mode, dq=acc, accumulate=True)
    assert_same(host(acc), prev + host(fresh), 'accumulate')            # (float32 + float32: one rounding)
    assert np.array_equal(gx0, gx2) and fresh.abs().max() > 0


class Guarded:
    """A buffer of `count` elements between two guard bands, all of it pre-filled with a sentinel BYTE and compared as bytes (so
    that any float pattern, a NaN included, compares)."""

    def __init__(self, dev, count, dtype, sentinel):
        self.item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = count * self.item
        assert self.nbytes % 16 == 0
        self.raw = torch.full((GUARD + self.nbytes + GUARD,), sentinel, dtype=torch.uint8, device=dev)
        self.view = self.raw[GUARD:GUARD + self.nbytes].view(dtype)
        self.sentinel = sentinel
        assert self.view.data_ptr() % 16 == 0

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def guards_intact(self):
        raw = self.raw.cpu().numpy()
        return bool((raw[:GUARD] == self.sentinel).all() and (raw[GUARD + self.nbytes:] == self.sentinel).all())

    def bytes(self):
        return self.raw[GUARD:GUARD + self.nbytes].cpu().numpy()


def run_guarded(dev, lib, shape, x, gy, q, sentinel):
    """Forward (soft, every output), backward and backward with the table gradient through the C ABI, every output and the workspace
    a view between guard bands -> ({name: bytes}, {name: guards intact})."""
    n, h, w = shape
    px, co = n * h * w, n * 3 * (h // 8) * (w // 8) * 64
    need = int(lib.nimg_djpeg_dq_workspace_bytes(n, h, w))
    assert need == (C.tasks_of(shape) + C.WAVES - 1) // C.WAVES * C.WAVES * 128 * 4
    bufs = dict(y=Guarded(dev, px * 3, torch.float32, sentinel), mask=Guarded(dev, px, torch.uint8, sentinel),
                idx=Guarded(dev, co, torch.int16, sentinel), xdq=Guarded(dev, co, torch.float32, sentinel),
                gx=Guarded(dev, px * 3, torch.float32, sentinel), gx_dq=Guarded(dev, px * 3, torch.float32, sentinel),
                dq=Guarded(dev, 128, torch.float32, sentinel), ws=Guarded(dev, need, torch.uint8, sentinel))
    xt, gyt, qt = g(x, dev), g(gy, dev), g(q, dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.nimg_djpeg_fwd(P(xt), bufs['y'].ptr(), P(qt), bufs['mask'].ptr(), bufs['idx'].ptr(), bufs['xdq'].ptr(),
                              n, h, w, 1, st) == 0
    assert lib.nimg_djpeg_bwd(P(xt), P(gyt), bufs['mask'].ptr(), P(qt), bufs['gx'].ptr(), n, h, w, 1, st) == 0
    assert lib.nimg_djpeg_bwd_dq(P(xt), P(gyt), bufs['mask'].ptr(), P(qt), bufs['gx_dq'].ptr(), bufs['dq'].ptr(), n, h, w, 1, 0,
                                 bufs['ws'].ptr(), need, st) == 0
    torch.cuda.synchronize(dev)
    return {k: b.bytes() for k, b in bufs.items()}, {k: b.guards_intact() for k, b in bufs.items()}


@pytest.mark.parametrize('tab', ['q50', 'frac'])
@pytest.mark.parametrize('case', GUARD_CASES)
def test_guard_bands_and_every_element_written(dev, case, tab):
    """Nothing is written outside an output or the exactly-sized workspace, every element inside is written (two runs over two
    different sentinels agree byte for byte - an element left alone would keep two different values - and the workspace, idle
    waves' slabs included, holds no sentinel word), and the outputs are the ones ops returns."""
    from neural_imaging_amd import _lib
    lib = _lib.load()
    shape = C.CASES[case]
    x, gy, q = C.images(shape, 'saturated'), C.gradient(shape), C.table(tab)
    a, guards_a = run_guarded(dev, lib, shape, x, gy, q, 0xA5)
    b, guards_b = run_guarded(dev, lib, shape, x, gy, q, 0x7F)
    assert all(guards_a.values()) and all(guards_b.values()), (guards_a, guards_b)
    for k in a:
        assert np.array_equal(a[k], b[k]), '{}: two runs over different sentinels differ - an element was not written'.format(k)
    ref = C.hard_reference(case, 'saturated', tab)
    assert np.array_equal(a['y'].view(np.float32).reshape(ref['y'].shape), ref['y'])
    assert np.array_equal(a['mask'].reshape(ref['mask'].shape), ref['mask'])
    assert np.array_equal(a['idx'].view(np.int16).reshape(ref['idx'].shape), ref['idx'])
    assert np.array_equal(a['xdq'].view(np.float32).reshape(ref['xd'].shape), ref['xd'])
    dq_t = torch.zeros((2, 8, 8), device=dev)
    gx = backward(dev, x, gy, ref['mask'], q, 'soft')
    gx_dq = backward(dev, x, gy, ref['mask'], q, 'soft', dq=dq_t)
    assert np.array_equal(a['gx'].view(np.float32).reshape(gx.shape), gx)
    assert np.array_equal(a['gx_dq'].view(np.float32).reshape(gx.shape), gx_dq)
    assert np.array_equal(a['dq'].view(np.float32).reshape(2, 8, 8), host(dq_t))
    # the slabs of the idle waves are zeros, not leftovers: the reduction adds every slab of the rounded-up workspace
    slabs = a['ws'].view(np.float32).reshape(-1, 128)
    assert slabs.shape[0] % C.WAVES == 0 and not slabs[C.tasks_of(shape):].any()
    assert np.isfinite(slabs).all()


@pytest.mark.parametrize('case', ['three-strips', 'full+ragged'])
def test_repeats_and_image_alone(dev, case):
    """Two runs give the same bits; an image run alone gives the bits it gives inside its batch."""
    shape = C.CASES[case]
    x, gy, q = C.images(shape, 'saturated'), C.gradient(shape), C.table('frac')

    def run(xs, gys):
        out = forward(dev, xs, q, 'soft')
        dq_t = torch.zeros((2, 8, 8), device=dev)
        out['gx'] = backward(dev, xs, gys, out['mask'], q, 'soft')
        out['gx_dq'] = backward(dev, xs, gys, out['mask'], q, 'soft', dq=dq_t)
        out['dq'] = host(dq_t)
        return out

    a, b = run(x, gy), run(x, gy)
    for k in a:
        assert_same(a[k], b[k], 'second run: ' + k)
    for i in range(shape[0]):
        one = run(x[i:i + 1], gy[i:i + 1])
        for k in ('y', 'mask', 'idx', 'xd', 'gx', 'gx_dq'):
            assert_same(one[k][0], a[k][i], 'image {} alone: {}'.format(i, k))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. the sub-sampled kernels' forward mask
def sub_forward(dev, sub, ref, mode):
    from neural_imaging_amd import ops
    hs, vs = C.SUB[sub]
    y, mask, (il, ic), _ = ops.djpeg_sub_fwd(g(ref['x'], dev), g(C.ijg(50), dev), mode, hs, vs, want_idx=True)
    return host(y), host(mask), host(il), host(ic)


def sub_left_out(sub, ref, mode, il, ic):
    """(n,h,w,3) bits that are left out: within 1e-5 of 0 or 1 in float64 and, for the hard modes, the pixels that read a block whose
    index flipped against float64 (the halo test_gpu_djpeg_sub.test_forward_hard_modes computes), capped like there."""
    from test_gpu_djpeg_sub import chroma_halo_pixels
    hs, vs = C.SUB[sub]
    out = C.near_edge(ref['pre'], C.EDGE_SMOOTH)
    if mode in C.HARD_MODES:
        fl, fc = il != ref['idx'][0], ic != ref['idx'][1]
        assert (fl.sum() + fc.sum()) / float(fl.size + fc.size) < 1e-4
        bad = np.kron(fl.any(axis=(3, 4)).astype(np.uint8), np.ones((1, 8, 8), np.uint8)).astype(bool)
        bad |= chroma_halo_pixels(fc.any(axis=(1, 4, 5)), hs, vs)
        out = out | bad[..., None]
    return out


@pytest.mark.parametrize('sub,shape,mode,kind', C.SUB_RUNS, ids=C.SUB_RUN_IDS)
def test_sub_forward_mask(dev, sub, shape, mode, kind):
    ref = C.sub_reference(sub, shape, mode, kind)
    assert C.CLIP_SHARE[0] <= C.clear_share(ref['mask'])
    if C.edge_cap_holds(mode, kind):
        assert C.near_edge(ref['pre'], C.EDGE_SMOOTH).mean() <= C.EDGE_CAP
    y, mask, il, ic = sub_forward(dev, sub, ref, mode)
    out = sub_left_out(sub, ref, mode, il, ic)
    assert_mask_two_sided(mask, ref['mask'], out, 'sub-sampled mask {} {} {} {}'.format(sub, shape, mode, kind))
    assert np.abs(y - ref['y'])[~out].max() <= ATOL


@pytest.mark.parametrize('sub,shape,mode,kind', C.SUB_RUNS, ids=C.SUB_RUN_IDS)
def test_sub_backward_with_the_kernels_mask(dev, sub, shape, mode, kind):
    """The mask the forward kernel wrote goes into the backward kernel.  Reference: autograd of the restatement at the float64 mask,
    the bits that were left out of the forward comparison (and only those) taken as the kernel decided them - a gradient spreads
    over its block, so leaving pixels out of the comparison of gx instead would hide whole blocks.  Every pixel is compared."""
    from neural_imaging_amd import ops
    hs, vs = C.SUB[sub]
    ref = C.sub_reference(sub, shape, mode, kind)
    gy = C.gradient(shape, seed=32)
    y, mask, il, ic = sub_forward(dev, sub, ref, mode)
    out = sub_left_out(sub, ref, mode, il, ic)
    assert_mask_two_sided(mask, ref['mask'], out, 'sub-sampled mask')
    keep = np.where(out, bits_to_keep(mask), bits_to_keep(ref['mask'])).astype(np.uint8)
    merged = (keep[..., 0] | keep[..., 1] << 1 | keep[..., 2] << 2).astype(np.uint8)
    assert np.array_equal(merged, mask)                   # (what the two-sided comparison above established)
    gx_ref = C.sub_backward_reference(sub, shape, mode, kind, gy, merged)
    gx = host(ops.djpeg_sub_bwd(g(ref['x'], dev), g(gy, dev), g(mask, dev, np.uint8), g(C.ijg(50), dev), mode, hs, vs))
    if mode == 'round':
        assert not gx_ref.any() and not gx.any()
    else:
        assert_close(gx, gx_ref, 1e-5, GRTOL * 3, what='sub-sampled djpeg bwd {} {} {} {}'.format(sub, shape, mode, kind))
