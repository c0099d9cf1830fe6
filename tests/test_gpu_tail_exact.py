"""
Everything between the FAN's last convolution and the updated weights - loss reductions, bias sums, FAN head, Adam, the DCN latent
- on EVERY route of its dispatch (cases and float64 reference halves: tests/tail_cases.py; operand rules: DESIGN.md section 5).

1. Bit for bit (test_*_exact).  Pixels k / 256 with differences j / 256, |j| <= 127: 255 d and its square are exact, the float64
   sum of the squares is exact in any order, so the loss must equal float32(s / count) with ==; the gradient is exact at the counts
   whose odd part divides 130050 (mse255) / 255 (mae255) - derivation in tail_cases.py.  Sums (bias_grad, gap, dense and fused-head
   gradients) run on small integers with sum |terms| < 2^24, bf16-stored operands within +-256 grid units, means over a
   power-of-two hw.  No operand or intermediate is a float32 denormal (asserted on the reference).
2. Adam: m and v bit for bit on dyadic gradients (tier 1); with the Keras constants the parameters, m and v lie within a
   per-element RUNNING ERROR BOUND computed in float64 next to the reference (tail_cases.adam_reference: unit roundoff 2^-24 times
   the roundings counted from adam_kernel's source) - no tuned tolerance.  adam_step_dev must be byte-identical to adam_step.
3. Softmax / cross-entropy and the latent (expf, logf, pow): the tolerances of tests/test_gpu_ops.py on every row of the dispatch.

Kernel reached by each test id (read off nimg_* in csrc/pointwise.hip, losses.hip, latent.hip, conv_wgrad.hip, head.hip):

  mse255_kernel / mae255_kernel / l2_loss_kernel     mse255-* / mae255-* / l2_loss-*: -n1 .. -n257 one or two workgroups; -n523776
        (l2: -n261888) one workgroup short of the grid cap, -n524288 (-n262144) the cap, +1 the first strided element, -n2080800
        (l2: -n798777) a ragged count four strides deep, -n12582912 the bench batch; -loss no gradient, -grad, -grad-acc
  mse255_final_kernel, mean_final_kernel, sum_final_kernel   the same ids (1 .. 2048 partials)
  mse255_sum_s2d3_rows_kernel       s2d3-rows-* (w = 2, 16, 510, 512; -nrows2560, -nrows8192: grid cap 2048 rows; -p1 .. -p6 parts)
  mse255_sum_s2d3_kernel            s2d3-pairs-oddw-* (odd w; -blocks: 510 workgroups), s2d3-pairs-w514-* (w > 512),
                                    s2d3_offset_operands (8-byte aligned operands), switched_s2d3 (NIMG_NO_S2D3_ROWS, child)
  add_kernel, add_n_kernel, lrelu_bwd_kernel   add-*, add_n-*, lrelu_bwd-* (counts around the cap, float4 items for add_n)
  bias_grad_partial_kernel          bias-generic-*: cpad 32 (cout 1, 3, 31), 64 (33), 128 (65), 256 (129, 257, 300: cb loop)
  bias_grad_partial4_kernel<false>  bias-float4-* (cout 4 .. 1024); -npix1048577 / -npix1228807: trailing empty workgroups
  bias_grad_partial4_kernel<true>   bias-bf16-*
  gap_fwd_kernel                    fan-vec-* (float4 route), fan-scalar-* (c = 6, 100, 1028), fan-hw225-*
  dense_softmax_ce_kernel / _wide   fan-*-k1 .. -k16 / -k17 .. -k256 (test_fan_softmax_routes)
  dense_bwd_params_kernel / _wide   fan-*-k1 .. -k16 / -k17 .. -k256 (test_fan_linear_exact, through fan_head_bwd AND fan_dense_bwd)
  gap_bwd_kernel                    fan-*-parts16 (n < 256), -parts4 (n = 256, 320), -parts1 (n = 1024); hw 16 / 64 / 256 against
                                    parts * ppi = 16 (c 1024), 64 (c 256), 512 (c 32)
  head_kernel<NW, NF, 0 | 1>, head_wgrad_kernel<NF, 64 | 128>, head_dact_kernel   head-n{1,5,320}-hw{64,128,256}-c{64,128,256}
  adam_kernel                       adam-tier1-*, adam-tier2-* (nimg_adam_step and nimg_adam_step_dev side by side), adam_skip_flag
  nan_flag_kernel                   nan_flag-*
  soft_codebook_fwd/bwd_win_kernel<K, 51>    latent-win{8,16,32}-*, latent-win*-probe, hist-*, data_parallel
  soft_codebook_fwd/bwd_fast_kernel<K, 51>   latent-fast{8,16,32}-m51-*; switched_latent[NIMG_LATENT_NO_WINDOW]
  soft_codebook_fwd/bwd_fast_kernel<K, 0>    latent-fast{8,16,32}-mint-* (v = 2: m = 3)
  soft_codebook_fwd/bwd_kernel<64|128|256>   latent-generic64-* (K = 5, 64; v = 2.5: pow()), -generic128-* (65, 128), -generic256-*
                                    (129, 256); latent-rounding-*; switched_latent[NIMG_LATENT_GENERIC | NIMG_LATENT_GENERIC_POW]
  hist_reduce_kernel, entropy_finalize_kernel, dscale_final_kernel   hist-nblocks{1,15,16,17,1024}, every latent id
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import tail_cases as C
from util import assert_close, assert_exact, err

pytestmark = pytest.mark.gpu

GRTOL = 1e-4                                  # tests/test_gpu_ops.py
_T0 = [None]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    _T0[0] = time.monotonic()
    yield torch.device('cuda', 0)
    print('tail: module wall time {:.1f} s'.format(time.monotonic() - _T0[0]))          # (shown with pytest -s)


def dv(a, dev, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(dev).contiguous()          # (np.array: always a copy)


def host(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def params(cases, prefix=''):
    return [pytest.param(c, id=prefix + c['name']) for c in cases]


# ----------------------------------------------------------------------------------------------------------------------
# 1. loss reductions
def _loss_op(ops, kind):
    if kind == 'l2_loss':                              # l2_loss(target, y): the gradient is taken at y
        return lambda a, b, **kw: ops.l2_loss(b, a, **kw)
    return getattr(ops, kind)


@pytest.mark.parametrize('case', params(C.LOSS_CASES))
def test_loss_exact(dev, case):
    from neural_imaging_amd import ops
    r = C.loss_case(case)
    kw = {}
    if case['grad']:
        kw['grad_scale'] = case['gscale']
        if case['acc']:
            kw.update(grad_out=dv(r['existing'], dev), accumulate=True)
    loss, grad = _loss_op(ops, case['kind'])(dv(r['a'], dev), dv(r['b'], dev), **kw)
    print('{}: loss {!r}, reference {!r}'.format(case['name'], float(loss.item()), float(r['loss'])))
    assert_exact(host(loss), [r['loss']], 'loss')
    if case['grad']:
        assert_exact(host(grad), r['grad'], 'gradient')
    else:
        assert grad is None


def _s2d3(ops, dev, r, case, offset=()):
    """offset: names of the operands placed 8 bytes into their allocation (16-byte alignment lost)."""
    def put(a, name):
        t = dv(a, dev)
        if name not in offset and 'all' not in offset:
            assert t.data_ptr() % 16 == 0
            return t
        buf = torch.empty(t.numel() + 2, device=dev)
        v = buf[2:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v
    parts = [put(p, 'part{}'.format(i)) for i, p in enumerate(r['parts'])]
    return ops.mse255_sum_s2d3(parts, put(r['a'], 'y'), put(r['b'], 'target'), case['gscale'])


@pytest.mark.parametrize('case', params(C.S2D3_CASES))
def test_s2d3_exact(dev, case):
    from neural_imaging_amd import ops
    r = C.s2d3_case(case)
    loss, dz = _s2d3(ops, dev, r, case)
    assert dz.shape == (case['n'], case['h'], case['w'], 12)
    assert_exact(host(dz), r['dz'], 'space_to_depth(sum(parts) + gk (y - target))')
    assert_exact(host(loss), [r['loss']], 'loss')


def test_s2d3_offset_operands(dev):
    """The same even-w shape on the row kernel (aligned) and on the pixel-pair kernel (an operand only 8-byte aligned: all of them,
    the target alone, the last part alone): identical bytes, equal to the reference."""
    from neural_imaging_amd import ops
    case = C.S2D3_SWITCH
    r = C.s2d3_case(case)
    loss0, dz0 = _s2d3(ops, dev, r, case)
    assert_exact(host(dz0), r['dz'], 'row kernel')
    assert_exact(host(loss0), [r['loss']], 'row kernel loss')
    for offset in (('all',), ('target',), ('part{}'.format(case['n_parts'] - 1),)):
        loss, dz = _s2d3(ops, dev, r, case, offset)
        assert torch.equal(dz, dz0) and torch.equal(loss, loss0), 'pixel-pair kernel ({} offset) differs from the row kernel'.format(offset)


@pytest.mark.parametrize('count', C.POINT_COUNTS)
def test_add_lrelu_bwd_exact(dev, count):
    from neural_imaging_amd import ops
    (a, b), ref = C.pointwise_case(count, 2)
    assert_exact(host(ops.add(dv(a, dev), dv(b, dev))), ref, 'add-n{}'.format(count))
    at = dv(a, dev)
    ops.add(at, dv(b, dev), out=at)
    assert_exact(host(at), ref, 'add in place')
    dy, y, want = C.lrelu_bwd_case(count)
    assert_exact(host(ops.lrelu_bwd(dv(dy, dev), dv(y, dev))), want, 'lrelu_bwd-n{}'.format(count))


@pytest.mark.parametrize('count', C.ADDN_COUNTS)
def test_add_n_exact(dev, count):
    from neural_imaging_amd import ops
    n = 2 + C.ADDN_COUNTS.index(count) % 5
    xs, ref = C.pointwise_case(count, n)
    assert_exact(host(ops.add_n([dv(x, dev) for x in xs])), ref, 'add_n-n{}-{} tensors'.format(count, n))
    xs6, ref6 = C.pointwise_case(count, 6)
    ts = [dv(x, dev) for x in xs6]
    ops.add_n(ts, out=ts[3])
    assert_exact(host(ts[3]), ref6, 'add_n of 6, in place')


# ----------------------------------------------------------------------------------------------------------------------
# bias sums
@pytest.mark.parametrize('case', params(C.BIAS_CASES))
def test_bias_grad_exact(dev, case):
    from neural_imaging_amd import ops
    r = C.bias_case(case)
    dz = dv(r['dz'], dev)
    if case['bf16']:
        dz = dz.to(torch.bfloat16)
    db = dv(r['existing'], dev) if case['acc'] else torch.full((case['cout'],), 7.0, device=dev)
    out = ops.bias_grad(dz, db=db, accumulate=case['acc'])
    assert out is db
    assert_exact(host(db), r['ref'], case['name'])
    if not case['acc']:
        assert_exact(host(ops.bias_grad(dz)), r['ref'], case['name'] + ', own output')


# ----------------------------------------------------------------------------------------------------------------------
# FAN head, generic path
@pytest.mark.parametrize('case', params(C.FAN_CASES))
def test_fan_linear_exact(dev, case):
    from neural_imaging_amd import ops
    r = C.fan_linear_case(case)
    n, c, k = case['n'], case['c'], case['k']
    act, w = dv(r['act'], dev), dv(r['w'], dev)
    gap, _, none1, none2 = ops.fan_head_fwd(act, w, torch.zeros(k, device=dev))
    assert none1 is None and none2 is None
    assert_exact(host(gap), r['gap'], 'gap')
    dlogits, loss_per = dv(r['dlogits'], dev), dv(r['loss_per'], dev)
    dw, db = torch.full((c, k), 7.0, device=dev), torch.full((k,), 7.0, device=dev)
    dact, loss = ops.fan_head_bwd(act, gap, w, dlogits, loss_per, r['loss_scale'], dw, db)
    assert_exact(host(dw), r['dw'], 'dw')
    assert_exact(host(db), r['db'], 'db')
    assert_exact(host(loss), [r['loss']], 'loss')
    assert_exact(host(dact), r['dact'], 'dact = (W dlogits) / hw * LeakyReLU\'(act)')
    dw2, db2 = torch.full((c, k), 7.0, device=dev), torch.full((k,), 7.0, device=dev)
    loss2 = ops.fan_dense_bwd(gap, dlogits, loss_per, r['loss_scale'], dw2, db2)
    assert torch.equal(dw2, dw) and torch.equal(db2, db) and torch.equal(loss2, loss)


@pytest.mark.parametrize('case', params([c for c in C.FAN_CASES if c['c'] <= 256], 'softmax-'))
def test_fan_softmax_routes(dev, case):
    """The tolerances of test_fan_head: 1e-6 probabilities, 1e-5 loss, GRTOL gradients."""
    from neural_imaging_amd import ops
    r = C.fan_softmax_case(case)
    n, c, k = case['n'], case['c'], case['k']
    act, w, b = dv(r['act'], dev), dv(r['w'], dev), dv(r['b'], dev)
    labels = torch.from_numpy(r['labels']).to(dev)
    gap, pr, lp, dl = ops.fan_head_fwd(act, w, b, labels, 1.0 / n)
    assert_close(host(pr), r['probs'], 1e-6, what='probs')
    pr2, lp2, dl2 = ops.fan_dense_fwd(gap, w, b, labels, 1.0 / n)
    assert torch.equal(pr2, pr) and torch.equal(lp2, lp) and torch.equal(dl2, dl)
    dw, db = torch.empty((c, k), device=dev), torch.empty((k,), device=dev)
    dact, lo = ops.fan_head_bwd(act, gap, w, dl, lp, 1.0 / n, dw, db)
    print('{}: loss {!r} vs {!r}; dw {}, db {}, dact {}'.format(case['name'], float(lo.item()), r['loss'], err(host(dw), r['dw']),
                                                                err(host(db), r['db']), err(host(dact), r['dact'])))
    assert abs(float(lo.item()) - r['loss']) < 1e-5
    assert_close(host(dw), r['dw'], 1e-6, GRTOL, what='dense dW')
    assert_close(host(db), r['db'], 1e-6, GRTOL, what='dense db')
    assert_close(host(dact), r['dact'], 1e-7, GRTOL, what='d pre-activation')


@pytest.mark.parametrize('case', params(C.FAN_HW225))
def test_fan_gap_of_a_15x15_map(dev, case):
    """hw = 225: the float4 route multiplies by 1 / hw, the scalar route divides by hw - both within the existing 1e-6."""
    from neural_imaging_amd import ops
    r = C.fan_softmax_case(case)
    gap, pr, _, _ = ops.fan_head_fwd(dv(r['act'], dev), dv(r['w'], dev), dv(r['b'], dev))
    assert_close(host(gap), r['gap'], 1e-6, what='gap')
    assert_close(host(pr), r['probs'], 1e-6, what='probs')


# ---- fused head
@pytest.mark.parametrize('case', params(C.HEAD_CASES + [C.HEAD_ZERO_CASE]))
def test_fused_head_exact(dev, case):
    from neural_imaging_amd import ops
    r = C.head_case(case)
    A, c = C.HEAD_ALPHA, case['c']
    ops.set_compute('bf16')
    try:
        x, w, b = dv(r['x'], dev).to(torch.bfloat16), dv(r['w'], dev), dv(r['b'], dev)
        assert ops.head_fused_ok(x, c)
        gap, mask, mask_p = ops.head_fwd(x, w, b, alpha=A)
        assert_exact(host(gap), r['gap'], 'gap')
        assert_exact(host(mask), r['mask'], 'mask words (channel-major)')
        assert_exact(host(mask_p), r['mask_p'], 'mask words (pixel-major)')
        if case['zero']:
            assert not np.array_equal(r['mask'], r['mask_inclusive']), 'no zero pre-activation in the zero-rule case'
        gap2, m2, mp2 = ops.head_fwd(x, w, b, want_mask=False, alpha=A)
        assert m2 is None and mp2 is None and torch.equal(gap2, gap)
        dl, wd = dv(r['dlogits'], dev), dv(r['wd'], dev)
        assert_exact(host(ops.head_dact(mask, dl, wd, x.shape, alpha=A)), r['dact'], 'head_dact')
        dw, db = torch.full((c, c), 7.0, device=dev), torch.full((c,), 7.0, device=dev)
        ops.head_wgrad(x, mask_p, dl, wd, dw, db, alpha=A)
        assert_exact(host(dw), r['dw'], 'head_wgrad dw')
        assert_exact(host(db), r['db'], 'head_wgrad db')
        dw1 = torch.full((c, c), 7.0, device=dev)
        ops.head_wgrad(x, mask_p, dl, wd, dw1, None, alpha=A)
        assert torch.equal(dw1, dw), 'head_wgrad without db'
        dw, db = dv(r['dw0'], dev), dv(r['db0'], dev)
        ops.head_wgrad(x, mask_p, dl, wd, dw, db, accumulate=True, alpha=A)
        assert_exact(host(dw), r['dw0'].astype(np.float64) + r['dw'], 'head_wgrad dw, accumulated')
        assert_exact(host(db), r['db0'].astype(np.float64) + r['db'], 'head_wgrad db, accumulated')
        assert_exact(host(ops.head_dgrad(mask, dl, wd, w, x, x.shape, alpha=A)), r['dx'], 'head_dgrad with in_mask')
        assert_exact(host(ops.head_dgrad(mask, dl, wd, w, None, x.shape, alpha=A)), r['dx_nomask'], 'head_dgrad without in_mask')
    finally:
        ops.set_compute('f32')


# ----------------------------------------------------------------------------------------------------------------------
# 2. Adam
def _adam_run(ops, dev, p0, grads, lr, b1, b2, eps, gscale):
    """len(grads) steps through nimg_adam_step and, side by side, nimg_adam_step_dev fed float32(the host's float64 lr_t): the two
    must agree in every byte after every step.  -> (p, m, v) numpy."""
    n = len(p0)
    st = [dv(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    st2 = [dv(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
    for k, g in enumerate(grads):
        gt = dv(g, dev)
        ops.adam_step(st[0], gt, st[1], st[2], lr, k + 1, b1, b2, eps, grad_scale=gscale)
        lr_t = torch.tensor([np.float32(ops.adam_lr_t(lr, k + 1, b1, b2))], dtype=torch.float32, device=dev)
        ops.adam_step(st2[0], gt, st2[1], st2[2], lr, k + 1, b1, b2, eps, grad_scale=gscale, lr_t_dev=lr_t)
        for a, b, name in zip(st, st2, 'pmv'):
            assert torch.equal(a, b), 'adam_step_dev differs from adam_step in {} at step {}'.format(name, k + 1)
    return [host(t) for t in st]


@pytest.mark.parametrize('gscale', [1.0, 0.5])
@pytest.mark.parametrize('count', C.ADAM_COUNTS)
def test_adam_tier1_state_exact(dev, count, gscale):
    from neural_imaging_amd import ops
    p0, grads, (p, m, v, Ep, Em, Ev) = C.adam_tier1_case(count, gscale)
    gp, gm, gv = _adam_run(ops, dev, p0, grads, 1e-3, 0.5, 0.75, 1e-7, gscale)
    assert_exact(gm, m, 'm')
    assert_exact(gv, v, 'v')
    C.assert_within_bound(gp, p, Ep, 'p')


@pytest.mark.parametrize('count,lr,gscale', [(n, 1e-3, 1.0) for n in C.ADAM_COUNTS] + [(257, 1e-4, 1.0), (C.CAP + 1, 1e-4, 0.5), (255, 1e-3, 0.3)])
def test_adam_tier2_within_the_running_bound(dev, count, lr, gscale):
    from neural_imaging_amd import ops
    p0, grads, pop = C.adam_populations(count, C._seed('adam2', count))
    p, m, v, Ep, Em, Ev = C.adam_reference(p0, grads, lr, 0.9, 0.999, 1e-7, gscale)
    gp, gm, gv = _adam_run(ops, dev, p0, grads, lr, 0.9, 0.999, 1e-7, gscale)
    for name, got, ref, bound in (('p', gp, p, Ep), ('m', gm, m, Em), ('v', gv, v, Ev)):
        ratio = np.abs(got - ref) / np.where(bound > 0, bound, 1.0)
        print('adam tier 2 n{} lr {} gscale {}: {} max |err| / bound {:.3f}'.format(count, lr, gscale, name, float(ratio.max())))
    C.assert_within_bound(gp, p, Ep, 'p')
    C.assert_within_bound(gm, m, Em, 'm')
    C.assert_within_bound(gv, v, Ev, 'v')
    zero = pop == 2
    assert np.array_equal(gp[zero], p0[zero]) and not gm[zero].any() and not gv[zero].any(), 'a zero gradient moved its parameter'


def test_adam_skip_flag(dev):
    from neural_imaging_amd import ops
    p0, grads, _ = C.adam_populations(C.CAP + 1, 5)
    g = dv(grads[0], dev)
    for dev_rate in (False, True):
        lr_t = torch.tensor([np.float32(ops.adam_lr_t(1e-3, 1))], device=dev) if dev_rate else None
        runs = {}
        for flag in (None, 0, 1):
            st = [dv(p0, dev), torch.full((len(p0),), 0.25, device=dev), torch.full((len(p0),), 0.5, device=dev)]
            fl = None if flag is None else torch.tensor([flag], dtype=torch.int32, device=dev)
            ops.adam_step(st[0], g, st[1], st[2], 1e-3, 1, skip_flag=fl, lr_t_dev=lr_t)
            runs[flag] = st
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[None])), 'a clear flag changed the step'
        assert not torch.equal(runs[None][0], dv(p0, dev))
        assert torch.equal(runs[1][0], dv(p0, dev)) and bool((runs[1][1] == 0.25).all()) and bool((runs[1][2] == 0.5).all())


@pytest.mark.parametrize('name,count,where,want', [pytest.param(*c, id='nan_flag-' + c[0]) for c in C.NAN_CASES])
def test_nan_flag(dev, name, count, where, want):
    from neural_imaging_amd import _lib, ops
    g = np.random.default_rng(count).standard_normal(count).astype(np.float32)
    g[::7] = np.inf
    g[3::11] = -np.inf
    if where is not None:
        g[where] = np.nan
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    gt = dv(g, dev)
    ops.nan_flag(gt, flag)
    assert int(flag.item()) == want
    flag.zero_()
    gt[0] = float('nan')
    assert _lib.load().nimg_nan_flag(gt.data_ptr(), 0, flag.data_ptr(), None) == 0        # a count of 0: no launch, no flag
    torch.cuda.synchronize()
    assert int(flag.item()) == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. latent
def _nearest(lat, cb):
    return np.argmin(np.abs(np.asarray(lat, np.float64)[:, None] - np.asarray(cb, np.float64)[None, :]), axis=1)


def _latent_check(ops, dev, r, K, v=50.0, unit=False, scale=None, soft=True, rounding='identity', what=''):
    """Forward + backward on one route against the oracle, with the tolerances of test_latent_soft_codebook_and_entropy;
    accumulate_dscale off (overwrites) and on."""
    tol = C.LAT_TOL
    ws = ops.LatentWorkspace(K, dev)
    sc = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
    z, cb, dl = dv(r['z'], dev), dv(r['cb'], dev), dv(r['dl'], dev)
    kw = dict(v=v, soft_codebook=soft, unit_codebook=unit, rounding=rounding)
    lat, ent = ops.latent_fwd(z, sc, cb, ws, **kw)
    if soft:
        assert np.array_equal(_nearest(host(lat), r['cb']), _nearest(r['latent'], r['cb'])), what + ': hard codebook indices differ'
    assert_close(host(lat), r['latent'], tol['latent'], what=what + ' latent')
    assert abs(float(ent.item()) - r['entropy']) < tol['entropy'], '{}: entropy {!r} vs {!r}'.format(what, float(ent.item()), r['entropy'])
    dscale = torch.full((1,), 3.0, device=dev)
    dz = ops.latent_bwd(z, sc, lat, dl, 250.0, cb, ws, dscale=dscale, **kw)
    print('{}: latent {:.2e}, entropy {:.2e}, dz {}, dscale rel {:.2e}'.format(
        what, err(host(lat), r['latent'])[0], abs(float(ent.item()) - r['entropy']), err(host(dz), r['dz']),
        abs(float(dscale.item()) - r['dscale']) / (abs(r['dscale']) + 1e-9)))
    assert_close(host(dz), r['dz'], tol['dz'][0], tol['dz'][1], what=what + ' dz')
    assert abs(float(dscale.item()) - r['dscale']) / (abs(r['dscale']) + 1e-9) < tol['dscale'], what + ' dscale'
    acc = torch.full((1,), 3.0, device=dev)
    dz2 = ops.latent_bwd(z, sc, lat, dl, 250.0, cb, ws, dscale=acc, accumulate_dscale=True, **kw)
    assert torch.equal(dz2, dz)
    assert float(acc.item()) == float(np.float32(3.0) + np.float32(dscale.item())), what + ': accumulate_dscale'
    return lat, ent, dz, dscale


@pytest.mark.parametrize('case', params(C.LATENT_CASES))
def test_latent_routes(dev, case):
    from neural_imaging_amd import ops
    _latent_check(ops, dev, C.latent_case(case), case['K'], case['v'], case['unit'], case['scale'], what=case['name'])


@pytest.mark.parametrize('case', params(C.LATENT_PROBE_CASES))
def test_latent_window_probe(dev, case):
    """K = 8 / 16: the five-centre window touches both ends of the codebook.  Windowed and full kernels against the oracle and
    each other (the comparisons of the existing K = 32 probe)."""
    from neural_imaging_amd import ops
    r = C.latent_probe_case(case)
    res = {unit: _latent_check(ops, dev, r, case['K'], 50.0, unit, None, what='{} unit={}'.format(case['name'], unit)) for unit in (False, True)}
    assert torch.equal(res[True][0], res[False][0]) and abs(float(res[True][1].item()) - float(res[False][1].item())) < 1e-7
    assert_close(host(res[True][2]), host(res[False][2]), 1e-9, 1e-6, what='windowed vs full dz')
    assert abs(float(res[True][3].item()) - float(res[False][3].item())) <= 1e-6 * abs(float(res[False][3].item())) + 1e-9


@pytest.mark.parametrize('case', params(C.LATENT_ROUNDING_CASES))
def test_latent_rounding_modes(dev, case):
    from neural_imaging_amd import ops
    r = C.latent_rounding_case(case)
    _latent_check(ops, dev, r, case['K'], 50.0, False, r['scale'], soft=False, rounding=case['rounding'], what=case['name'])
    _latent_check(ops, dev, r, case['K'], 50.0, True, r['scale'], soft=False, rounding=case['rounding'], what=case['name'] + ' (windowed)')


@pytest.mark.parametrize('nblocks', C.HIST_BLOCKS, ids=['hist-nblocks{}'.format(n) for n in C.HIST_BLOCKS])
def test_latent_histogram_of_known_answer(dev, nblocks):
    """z exactly on the centres with unequal counts: the latent is z, the histogram sums are the counts (every foreign weight is
    below 2e-33 of the own one) and the entropy is the closed form -sum q ln q / 0.6931 to the existing 1e-5."""
    from neural_imaging_amd import ops
    r = C.hist_case(nblocks)
    K = len(r['cb'])
    counts = np.bincount(r['idx'], minlength=K)
    for unit in (True, False):
        ws = ops.LatentWorkspace(K, dev)
        lat, ent = ops.latent_fwd(dv(r['z'], dev), None, dv(r['cb'], dev), ws, unit_codebook=unit)
        assert_exact(host(lat), r['z'], 'latent on the centres')
        hs = ws.hist_sums().cpu().numpy()
        print('hist-nblocks{} unit={}: entropy {!r} vs {!r}, max |hist - counts| {:.3e}'.format(
            nblocks, unit, float(ent.item()), r['entropy'], float(np.abs(hs - counts).max())))
        assert np.abs(hs - counts).max() <= 1e-9 * len(r['z']), 'histogram sums'
        assert abs(float(ent.item()) - r['entropy']) < 1e-5


def test_latent_data_parallel(dev):
    """Two halves into two workspaces (finalize = False), the K histogram sums added on the host, nimg_latent_entropy_finalize with
    count_global.  The latent is element-wise: byte-identical to the single pass.  Entropy and dz are NOT required byte-identical:
    the float64 histogram is summed per workgroup through LDS atomics of four waves (no fixed order) and the two halves cut the
    workgroups differently, so the sums agree to float64 rounding only - they are held to the tolerances of the single pass, and
    the two ranks (same sums, deterministic finalize) to each other byte for byte."""
    from neural_imaging_amd import ops
    case = dict(name='latent-win32-K32-dp', K=32, v=50.0, unit=True, count=70000, cb='unit', scale=1.3)
    r = C.latent_case(case)
    K, n, h = 32, case['count'], 33000
    lat1, ent1, dz1, _ = _latent_check(ops, dev, r, K, 50.0, True, 1.3, what='single pass')
    sc = torch.tensor([1.3], dtype=torch.float32, device=dev)
    z, cb, dl = dv(r['z'], dev), dv(r['cb'], dev), dv(r['dl'], dev)
    for accumulate in (False, True):
        wss, lats = [ops.LatentWorkspace(K, dev), ops.LatentWorkspace(K, dev)], []
        for ws, sl in zip(wss, (slice(0, h), slice(h, n))):
            lat, _ = ops.latent_fwd(z[sl], sc, cb, ws, count_global=n, finalize=False, unit_codebook=True)
            lats.append(lat)
        assert torch.equal(torch.cat(lats), lat1)
        total = wss[0].hist_sums().cpu() + wss[1].hist_sums().cpu()
        ents, dzs, ds = [], [], torch.full((1,), 2.0 if accumulate else 9.0, device=dev)
        for ws, sl, lat in zip(wss, (slice(0, h), slice(h, n)), lats):
            ws.hist_sums().copy_(total.to(dev))
            ent = torch.zeros(1, device=dev)
            ops.latent_entropy_finalize(ws, n, ent)
            ents.append(ent)
            dzs.append(ops.latent_bwd(z[sl], sc, lat, dl[sl], 250.0, cb, ws, dscale=ds, unit_codebook=True,
                                      accumulate_dscale=accumulate or sl.start > 0))
        assert torch.equal(ents[0], ents[1])
        dz = torch.cat(dzs)
        want_ds = r['dscale'] + (2.0 if accumulate else 0.0)
        print('data parallel: entropy {!r} vs single pass {!r} vs oracle {!r}; dz vs single pass {}; dscale {!r} vs {!r}'.format(
            float(ents[0].item()), float(ent1.item()), r['entropy'], err(host(dz), host(dz1)), float(ds.item()), want_ds))
        assert abs(float(ents[0].item()) - float(ent1.item())) < C.LAT_TOL['entropy'] and abs(float(ents[0].item()) - r['entropy']) < C.LAT_TOL['entropy']
        assert_close(host(dz), host(dz1), *C.LAT_TOL['dz'], what='dz vs the single pass')
        assert_close(host(dz), r['dz'], *C.LAT_TOL['dz'], what='dz vs the oracle')
        assert abs(float(ds.item()) - want_ds) / abs(want_ds) < C.LAT_TOL['dscale']


# ----------------------------------------------------------------------------------------------------------------------
# 4. the forms behind switches the library reads once per process: one child per switch, never retried
def _child(switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith('NIMG_')}
    env[switch] = '1'
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'tail_child.py')
    p = subprocess.run([sys.executable, child, switch], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
    assert p.returncode == 0, 'child failed ({}): {}'.format(p.returncode, p.stderr.decode()[-2000:])
    return dict(l.split(' ', 1) for l in p.stdout.decode().splitlines() if ' ' in l)


def _arr(lines, key, like, dtype=np.float32):
    return np.frombuffer(bytes.fromhex(lines[key].strip()), dtype=dtype).reshape(np.asarray(like).shape)


def test_switched_s2d3_in_a_fresh_process(dev):
    """NIMG_NO_S2D3_ROWS: the pixel-pair kernel at the even-w shapes the row kernel takes.  The row kernel runs here first; only
    when it passes, ONE child runs the pixel-pair kernel; its bytes must equal the row kernel's and the reference."""
    from neural_imaging_amd import ops
    here = {}
    for tag, case in (('a', C.S2D3_SWITCH), ('b', C.S2D3_SWITCH2)):
        r = C.s2d3_case(case)
        loss, dz = _s2d3(ops, dev, r, case)
        assert_exact(host(dz), r['dz'], 'in-process (row kernel)')
        assert_exact(host(loss), [r['loss']], 'in-process loss')
        here[tag] = (r, host(dz), host(loss))
    lines = _child('NIMG_NO_S2D3_ROWS')
    assert set(lines) == {'loss_a', 'dz_a', 'loss_b', 'dz_b'}, sorted(lines)
    for tag, (r, dz, loss) in here.items():
        got = _arr(lines, 'dz_' + tag, dz)
        assert_exact(got, r['dz'], 'child (pixel-pair kernel)')
        assert got.tobytes() == dz.tobytes() and _arr(lines, 'loss_' + tag, loss).tobytes() == loss.tobytes()


@pytest.mark.parametrize('switch', ['NIMG_LATENT_GENERIC', 'NIMG_LATENT_GENERIC_POW', 'NIMG_LATENT_NO_WINDOW'])
def test_switched_latent_in_a_fresh_process(dev, switch):
    """One K = 32 case per switch (generic kernel with the integer power, generic kernel with pow(), fast kernel without the window)
    against the same reference as the default (windowed) form, which runs here first."""
    from neural_imaging_amd import ops
    case, tol = C.LATENT_SWITCH, C.LAT_TOL
    r = C.latent_case(case)
    _latent_check(ops, dev, r, case['K'], case['v'], case['unit'], case['scale'], what='in-process (windowed)')
    lines = _child(switch)
    assert set(lines) == {'latent', 'entropy', 'dz', 'dscale'}, sorted(lines)
    lat, dz = _arr(lines, 'latent', r['latent']), _arr(lines, 'dz', r['dz'])
    ent, ds = float(_arr(lines, 'entropy', [0])[0]), float(_arr(lines, 'dscale', [0])[0])
    assert np.array_equal(_nearest(lat, r['cb']), _nearest(r['latent'], r['cb']))
    assert_close(lat, r['latent'], tol['latent'], what='child latent')
    assert abs(ent - r['entropy']) < tol['entropy']
    assert_close(dz, r['dz'], *tol['dz'], what='child dz')
    assert abs(ds - r['dscale']) / (abs(r['dscale']) + 1e-9) < tol['dscale']
