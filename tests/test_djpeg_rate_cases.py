"""
The references of the exact rate-term tests (tests/djpeg_rate_cases.py) checked on the CPU: the oracle's z, the analytic estimator
against float64 autograd of oracle.tfops.entropy, the unique / counts form against the plain one, the task counts and grids the cases
are named for, where codebook-sweep puts its values, the clip conditions of every run, and - printed - the floors and tolerances
that tests/test_gpu_djpeg_rate_exact.py holds the kernels to.
"""
import time

import numpy as np
import pytest
import torch

import djpeg_cases as C
import djpeg_rate_cases as R
from oracle import tfops as T
from util import to64


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('tab', ['q50', 'ones', 'frac', 'last'])
@pytest.mark.parametrize('case', ['three-strips', 'ragged-only'])
def test_oracle_z_is_the_quotient_behind_idx(case, tab):
    """djpeg_ref_forward_z shares forward_body: the old outputs keep their bits, rint(z) is idx, z * ... is not recomputed anywhere."""
    x, q = C.images(C.CASES[case], 'saturated'), C.table(tab)
    y, idx, xd = C.c_forward(x, q)
    out = C.c_forward_z(x, q)
    assert bits_equal(out['y'], y) and bits_equal(out['idx'], idx) and bits_equal(out['xd'], xd)
    z = out['z']
    assert z.dtype == np.float32 and z.shape == idx.shape and np.isfinite(z).all()
    assert np.array_equal(np.rint(z).astype(np.int16), idx)
    assert bits_equal(np.rint(z) * q[None, :, None, None, :, :], xd)
    z64 = torch.stack(C.restate64(to64(x), to64(q), 'identity')[2], 1).numpy()
    assert np.abs(z - z64).max() <= 4e-7 * np.abs(z64).max() + 1e-4          # float32 transform of values up to ~1000
    lib = C.clib()
    assert lib.djpeg_ref_forward_z(C._vp(x), C._vp(np.zeros_like(x)), C._vp(q), None, None, None, *x.shape[:3]) == 0
    assert lib.djpeg_ref_forward_z(C._vp(x), C._vp(np.zeros_like(x)), C._vp(q), None, None, None, 1, 8, 70) == -1


def test_linear_part_is_restate64s():
    x = to64(C.images((2, 16, 56), 'noise'))
    z = torch.stack(C.restate64(x, torch.ones(3, 8, 8, dtype=torch.float64), 'identity')[2], 1)
    assert torch.equal(R.linear_X(x), z)
    # the adjoint is the adjoint: <X(x) - X(0), G> == <x, adjoint(G)>
    G = np.random.default_rng(4).normal(size=tuple(z.shape))
    lhs = float(((R.linear_X(x) - R.linear_X(torch.zeros_like(x))) * torch.from_numpy(G)).sum())
    rhs = float((x.numpy() * R.adjoint(G, tuple(x.shape))).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize('mode', ['sin', 'harmonic', 'soft', 'round', 'identity'])
def test_quantiser_and_surrogate_are_the_models(mode):
    z = C.c_forward_z(C.images((1, 8, 72), 'noise'), C.table('frac'))['z']
    zt = to64(z).requires_grad_(True)
    et = T.quantization(zt, mode)
    e = R.quantise(mode, z)
    assert e.dtype == np.float32
    assert np.abs(e - et.detach().numpy()).max() <= 0.5 * np.spacing(np.abs(e)).max()        # the float64 formula, rounded once
    et.sum().backward()
    assert np.abs(R.surrogate(mode, z) - zt.grad.numpy()).max() <= 1e-9                      # 2 pi z of z up to a few hundred


AUTOGRAD_RUNS = [('one-block', 'saturated', 'q50', 'sin'), ('ragged-only', 'noise', 'frac', 'identity'),
                 ('one-block', 'saturated', 'ones', 'harmonic')]          # the last: values far out of range


@pytest.mark.parametrize('case,kind,tab,mode', AUTOGRAD_RUNS, ids=['-'.join(r) for r in AUTOGRAD_RUNS])
def test_analytic_estimator_equals_autograd(case, kind, tab, mode):
    """H, g_k = dH / d mean_k and dH / de of the analytic form against torch float64 autograd of oracle.tfops.entropy on the same
    e, to 1e-12 of their maxima."""
    e = R.quantise(mode, C.c_forward_z(R.inputs(case, kind), R.table(tab))['z'])
    est = R.estimator(e)
    et = to64(e).reshape(-1).requires_grad_(True)
    cb = torch.from_numpy(R.CODEBOOK)
    H = T.entropy(et, cb, R.V, R.GAMMA)[0]
    H.backward()
    H = H.detach()
    assert abs(est['H'] - float(H)) <= 1e-12 * abs(float(H))
    de = et.grad.numpy().reshape(e.shape)
    assert np.abs(de).max() > 0
    assert np.abs(est['dde'] / est['N'] - de).max() <= 1e-12 * np.abs(de).max()
    # g_k: the lines of entropy() from the mean histogram on, the mean as the leaf
    hm = T._codebook_weights(to64(e).reshape(-1), cb, R.V, R.GAMMA).mean(dim=0).detach().requires_grad_(True)
    hc = torch.clamp(hm, min=1e-9)
    hn = hc / hc.sum()
    H2 = -(hn * torch.log(hn)).sum() / 0.6931
    assert float(H2.detach()) == float(H)
    H2.backward()
    assert np.abs(est['hm'] - hm.detach().numpy()).max() <= 1e-12 * float(hm.detach().max())
    assert np.abs(est['g'] - hm.grad.numpy()).max() <= 1e-12 * np.abs(hm.grad.numpy()).max()
    if tab == 'ones':
        assert (~R.in_range(e)).any()


@pytest.mark.parametrize('mode', ['sin', 'round'])
def test_unique_counts_form_equals_the_plain_form_on_a_tiled_input(mode):
    base, q = C.images((3, 8, 16), 'saturated'), R.table('q50')
    index = np.arange(10) % 3
    tiled = R.reference_from(base, index, q, mode)
    flat = R.reference_from(base[index], np.arange(10), q, mode)
    plain = R.estimator_plain(R.quantise(mode, C.c_forward_z(base[index], q)['z']))
    assert tiled['N'] == flat['N'] == plain['N'] == 10 * 8 * 16 * 3
    assert tiled['distinct'] <= 3 * 8 * 16 * 3
    for other in (flat, plain):
        assert abs(tiled['H'] - other['H']) <= 1e-12 * abs(other['H'])
        assert np.abs(tiled['g'] - other['g']).max() <= 1e-12 * np.abs(other['g']).max()
    assert np.abs(tiled['gx'][index] - flat['gx']).max() <= 1e-12 * np.abs(flat['gx']).max()
    assert np.abs(tiled['dq'] - flat['dq']).max() <= 1e-12 * np.abs(flat['dq']).max()
    if mode == 'round':
        assert not tiled['gx'].any() and not tiled['dq'].any()
    else:
        assert tiled['gx'].any() and tiled['dq'].any()


def test_task_counts_and_grids():
    assert {k: R.grid_of(R.CASES[k]) for k in ('seg-31', 'seg-32', 'seg-33', 'grid-cap')} == \
        {'seg-31': 31, 'seg-32': 32, 'seg-33': 33, 'grid-cap': 1024}
    assert R.tasks_of(R.CASES['seg-32']) == 31 * 4 + 1                      # the last workgroup has one live wave
    assert R.tasks_of(R.CASES['grid-cap']) == 4112 == 4096 + 16
    assert R.waves_with_two_tasks(R.CASES['grid-cap']) == 16
    assert all(R.waves_with_two_tasks(s) == 0 for k, s in R.CASES.items() if k != 'grid-cap')
    assert max(R.grid_of(s) for k, s in R.CASES.items() if k in C.CASES) <= 3      # what the strip cases reach
    assert all(3 * n * h * w <= 25000 for n, h, w in (R.CASES[k] for k in ('seg-31', 'seg-32', 'seg-33')))
    # grid-cap: 7 distinct images, a full strip and a one-block strip each; its second-iteration tasks are images 2048 .. 2055
    base, index = R.batch('grid-cap', 'saturated')
    assert base.shape == (7, 8, 72, 3) and index.shape == (2056,) and len({b.tobytes() for b in base}) == 7
    assert 4096 // 2 == 2048 and np.array_equal(index[2048:], np.arange(2048, 2056) % 7)
    assert [C.is_integer_table(R.table(t)) for t in ('sweep-int', 'sweep-frac')] == [True, False]
    assert len(set(R.RUN_IDS)) == len(R.RUNS)
    assert {r[3] for r in R.RUNS} == set(R.MODES)
    assert {r[3] for r in R.RUNS if r[0] == 'grid-cap'} == {'round', 'sin', 'identity'}
    for case in R.ROUTE_CASES + ['codebook-sweep']:
        got = {(r[3], C.is_integer_table(R.table(r[2]))) for r in R.RUNS if r[0] == case}
        assert got >= {(m, i) for m in R.MODES for i in (True, False)}, case


def test_grid_cap_reference_is_cheap():
    t0 = time.time()
    ref = R.reference_from(*R.batch('grid-cap', 'saturated'), R.table('q50'), 'sin')
    dt = time.time() - t0
    print('grid-cap sin: {} distinct values of {:.0f}, reference and floors in {:.2f} s'.format(ref['distinct'], ref['N'], dt))
    assert ref['N'] == 2056 * 8 * 72 * 3 and 12000 <= ref['distinct'] <= 12096


def test_codebook_sweep_reaches_the_ends_of_the_code_book():
    seen = {}
    for tab in R.SWEEP_DC:
        e = R.reference('codebook-sweep', 'sweep', tab, 'identity')['e']
        inside, k0 = R.in_range(e), R.nearest_centre(e)
        seen[tab] = {k for k in (0, 1, 510, 511) if ((k0 == k) & inside).any()}
        zero = float(((k0 == 255) & inside).mean())
        print('{}: truncated windows at {}, {} below, {} above, {} ballot rounds with two lanes out of range, {:.1%} at the zero '
              'centre'.format(tab, sorted(seen[tab]), int((e < -255.5).sum()), int((e > 256.5).sum()),
                              R.strips_with_two_out_of_range(e), zero))
        assert zero >= 0.10 and 1.0 - zero >= 0.10
        assert (e > 256.5).any()
        assert np.abs(e).max() < 256.0 + R.FAR_BEYOND
    assert seen['sweep-int'] >= {1, 511} and seen['sweep-frac'] >= {0, 510}          # k0 = 0 needs a value under -254.5: 3.96 only
    e = R.reference('codebook-sweep', 'sweep', 'sweep-frac', 'identity')['e']
    assert (e < -255.5).any() and (e > 256.5).any() and R.strips_with_two_out_of_range(e) >= 1
    # the luma DC of the last strip: levels 254 and 255, neighbouring blocks, both above the range
    assert e[0, 0, 15, 14, 0, 0] > 256.5 and e[0, 0, 15, 15, 0, 0] > 256.5 and e[0, 0, 0, 0, 0, 0] < -255.5


@pytest.mark.parametrize('case,kind,tab,mode', R.RUNS, ids=R.RUN_IDS)
def test_clip_conditions_and_floors(case, kind, tab, mode):
    """Every run: at least three bins above the 1e-9 clip and at least one under it (a wrong clip mask shows in g), and no bin
    within 1 % of the clip (there float64 rounding may decide it either way).  A condition on the inputs: a run that breaks it
    gets another seed.  The floors and tolerances of the GPU comparison are printed."""
    ref = R.reference(case, kind, tab, mode)
    print(R.describe(case, kind, tab, mode, ref))
    hm = ref['hm']
    unclipped = int((hm >= R.CLIP).sum())
    assert unclipped >= 3
    assert not (np.abs(hm / R.CLIP - 1.0) <= 0.01).any()
    if (case, kind, tab) == R.FAR_RUN:
        assert np.abs(ref['e']).max() >= 256.0 + R.FAR_BEYOND and ref['N'] < 1.0 / (512 * R.CLIP) and unclipped == 512
    else:
        assert unclipped <= 511
    assert np.isfinite(ref['gx']).all() and np.isfinite(ref['dq']).all() and np.isfinite(ref['g']).all()
    if mode == 'round':
        assert not ref['gx'].any() and not ref['dq'].any()
    else:
        assert ref['gx'].any() and ref['dq'].any()
        assert 0 < ref['tol_gx'] < 3.4e-2 and 0 < ref['tol_dq'] < 3.4e-2        # (the old tolerances were 1e-3 .. 3.4e-2)
    assert (ref['g'][hm < R.CLIP] == 0).all() and (ref['g'][hm >= R.CLIP] != 0).all()
