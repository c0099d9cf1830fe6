"""
The glue between the convolutions, the image chain and the tail of the step - pooling and un-pooling, the depth-to-space heads, the
float32 transposed convolution, the element-wise streams, dropout, the confusion matrix, the constrained-filter normalisation and
the SSIM / MS-SSIM family - on EVERY route of its dispatch (cases and float64 reference halves: tests/glue_cases.py; operand
rule: DESIGN.md section 5; the CPU self-test of the comparisons: tests/test_glue_helpers.py).

1. Bit for bit (assert_exact).  Small integers or k / 256 (k / 4096 for the clip heads), scales 1, 1/2, 1/4, shifts 0, 1/2,
   LeakyReLU with alpha = 1/4: every product and sum is a float32 number (asserted on the reference), so a contraction to fma cannot
   matter; bf16-stored operands keep 8 significant bits.  Routing kernels get operands whose elements all differ; arg-max bytes
   hold all four values in every channel lane of an 8-channel granule.
2. expf / tanhf / powf streams: the tolerances of tests/test_gpu_ops.py::test_classic_isp_pointwise, plus the saturated ends.
3. SSIM family: values to the project's 1e-5, gradients to the bound of test_image_losses_with_gradient, the float32 derivative
   maps to 2^-23 |ref| + 1e-12 against float64 restatements that read the very float32 window the library holds.

Kernel reached by each test id (read off nimg_* in csrc/pointwise.hip, latent.hip, isp.hip, constrained.hip, losses.hip):

  maxpool2_fwd_kernel<4> / <1> / maxpool2_fwd_bf16_kernel   maxpool2<4>-* (c 4, 32) / maxpool2<1>-* (c 1, 3, 6) / maxpool2-bf16-*
        (c 8, 24); odd h, odd w, both; -above-cap: more than 2048 * 256 items
  maxpool2_bwd_kernel<4> / <1> / maxpool2_bwd_bf16_kernel   maxpool2_bwd-f32<4>-* / -f32<1>-* / -bf16-*: add none / separate / in place
        x mask on / off; odd sizes: -add_none (the dropped row and column are 0), -add_separate (raises), -add_inplace
  maxpool2_bwd_border_kernel        maxpool2_bwd-*-{7x8,6x9,5x7,3x3}-add_inplace-mask (the dropped row / column under the mask)
  maxpool2_unpool_bf16x8_kernel     unpool-x8-* (c 8, 16; -above-cap), unpool_x8_equals_generic
  maxpool2_unpool_kernel<IN, OUT>   unpool-<true,true>-* (c 12; the mask at c 8), -<true,false>-*, -<false,true>-*, -<false,false>-*
  d2s_clip3_fwd / _bwd_kernel       d2s_clip3-* / d2s_clip3_bwd-* (2x6x5x12, 1x1x1x12, 1x725x725x12 above the cap)
  d2s_clip4_fwd / _bwd_kernel       d2s_clip4-* / d2s_clip4_bwd-* (co 4, 8, 32, 128; 1x363x363x16 above the cap)
  d2s_clip_fwd / _bwd_kernel        d2s_generic-* / d2s_generic_bwd-* (co 1, 2, 5).  NOT REACHED at co % 4 == 0: that needs
        n h w co >= 2^32 - 2048 * 256 elements
  d2s2_scale3_kernel / d2s2_scale_kernel   d2s2_scale3-c3-cp16-* / d2s2_scale-c{1,4,3}-cp{4c, 4c + 4}-*
  zero_insert2_kernel               zero_insert2-*
  convt2x2_fwd_kernel               convt2x2_f32-* (cin 12, 24, 33, 64 x cout 4, 40, 65, 128; 1, 15, 16, 17, 35 pixels;
        -under-bf16-*: throughput mode with cin % 8 != 0 or cout < 8 reaches the same kernel)
  add_kernel, add_n_kernel          add_streams-n* (2..6 inputs, out aliasing each input; pairwise fallback at 7 inputs, at
        count % 4 != 0 and on a 4-byte-offset view)
  lrelu_bwd_kernel, lrelu_fwd_kernel, affine_kernel, clip01_kernel, int_words_kernel, float_fill_kernel   simple_streams-n*
  mask_scale_kernel                 mask_scale-n*
  activation_fwd_kernel<0 | 1>, activation_bwd_kernel<0 | 1>   activation_exact-n*
  residual_fwd_kernel               isp_residual-n*
  residual_bwd_kernel, residual_final_kernel   isp_residual_bwd-n* (n262149: the second trip past RED_BLOCKS)
  constrained_fwd_kernel, constrained_bwd_kernel   constrained-ks{3,5,7}-c{1,3,16}-*, constrained_random_float, constrained_refuses_17
  confusion_kernel                  confusion-k{1,2,7}-n{1,255,257,5000}
  tanh_fwd / tanh_bwd_kernel, sigmoid_fwd / _bwd_kernel, gamma_ste_fwd / _bwd_kernel, activation_fwd / _bwd_kernel<2 | 3 | 4>
                                    transcendental-n*, saturated_ends
  ssim_partial_kernel<7> / <11>, ssim_final_kernel   ssim<7>-* / ssim<11>-* (ho, wo in 1, 16, 17; -above-64-tiles), ssim_constant_images
  ssim_loss_stats_kernel, ssim_loss_grad_kernel, mean_final_kernel   ssim_loss-* (h, w in 11, 12, 21, 22; 90x90x3: more than 64 * 256
        items per image; max_val 255)
  ssim_planes_kernel, ssim_planes_final_kernel   ssim_planes-* (which 0, 1, 2; 70 planes; 47 x 48 positions per plane), msssim_end_to_end
  msssim_combine_kernel             msssim_combine-p{1,64,65,130}-*
  ssim_loss_grad_kernel with coef   ssim_maps_grad
"""
import time

import numpy as np
import pytest
import torch

import glue_cases as C
from util import assert_close, assert_exact, to64

pytestmark = pytest.mark.gpu

A = C.ALPHA
_T0 = [None]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    _T0[0] = time.monotonic()
    yield torch.device('cuda', 0)
    print('glue: module wall time {:.1f} s'.format(time.monotonic() - _T0[0]))          # (shown with pytest -s)


def dv(a, dev, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype, order='C')).to(dev).contiguous()          # (np.array: always a copy)


def host(t):
    return t.float().cpu().numpy() if t.dtype == torch.bfloat16 else t.cpu().numpy()


def params(cases):
    return [pytest.param(c, id=c['name']) for c in cases]


def stored(a, dev, bf16):
    t = dv(a, dev)
    return t.to(torch.bfloat16) if bf16 else t


# ----------------------------------------------------------------------------------------------------------------------
# A. pooling
@pytest.mark.parametrize('case', params(C.MAXPOOL_CASES))
def test_maxpool2(dev, case):
    from neural_imaging_amd import ops
    r = C.maxpool_case(case)
    y = ops.maxpool2(stored(r['x'], dev, case['bf16']))
    assert y.dtype == (torch.bfloat16 if case['bf16'] else torch.float32)
    assert_exact(host(y), r['ref'], case['name'])


@pytest.mark.parametrize('case', params(C.MAXPOOL_BWD_CASES))
def test_maxpool2_bwd(dev, case):
    from neural_imaging_amd import ops
    r = C.maxpool_bwd_case(case)
    b = case['bf16']
    dp, yact = stored(r['dp'], dev, b), stored(r['yact'], dev, b)
    if case['add'] == 'none':
        out = torch.full_like(yact, 7.0)                      # (stale contents: the dropped row / column must come out 0)
        dz = ops.maxpool2_bwd(dp, yact, None, apply_mask=case['mask'], out=out, alpha=A)
        assert dz is out
    elif case['add'] == 'separate':
        add = stored(r['add'], dev, b)
        if r['raises']:
            with pytest.raises(RuntimeError):
                ops.maxpool2_bwd(dp, yact, add, apply_mask=case['mask'], alpha=A)
            return
        dz = ops.maxpool2_bwd(dp, yact, add, apply_mask=case['mask'], alpha=A)
        assert_exact(host(add), r['add'], 'the separate add operand is left alone')
    else:                                                     # the UNet's production call: the skip gradient is the output buffer
        buf = stored(r['add'], dev, b)
        dz = ops.maxpool2_bwd(dp, yact, add=buf, apply_mask=case['mask'], out=buf, alpha=A)
        assert dz is buf
    assert_exact(host(dz), r['ref'], case['name'])


def _unpool(ops, dev, r, mask, alpha=A):
    dp = stored(r['dp'], dev, r['in_bf16'])
    return ops.maxpool2_unpool(dp, dv(r['idx'], dev, np.uint8), dv(r['pooled'], dev), apply_mask=mask, out_bf16=r['out_bf16'],
                               alpha=alpha)


@pytest.mark.parametrize('case', params(C.UNPOOL_CASES))
def test_maxpool2_unpool(dev, case):
    from neural_imaging_amd import ops
    r = C.unpool_case(case)
    dz = _unpool(ops, dev, r, case['mask'])
    assert dz.dtype == (torch.bfloat16 if r['out_bf16'] else torch.float32)
    assert_exact(host(dz), r['ref'], case['name'])


@pytest.mark.parametrize('case', params([c for c in C.UNPOOL_CASES if c['form'] == 'x8' and not c['big']]))
def test_unpool_x8_equals_generic(dev, case):
    """The packed form must be byte-identical to maxpool2_unpool_kernel<true, true> on the same operands: that kernel is reached
    with the mask on and alpha = 1 (a float32 multiplication by exactly 1)."""
    from neural_imaging_amd import ops
    r = C.unpool_case(case)
    x8 = _unpool(ops, dev, r, False)
    generic = _unpool(ops, dev, r, True, alpha=1.0)
    assert x8.dtype == generic.dtype == torch.bfloat16
    assert torch.equal(x8.view(torch.int16), generic.view(torch.int16))


# ----------------------------------------------------------------------------------------------------------------------
# B. layout
@pytest.mark.parametrize('case', params(C.D2S_CASES))
def test_d2s_clip(dev, case):
    from neural_imaging_amd import ops
    r = C.d2s_case(case)
    y = ops.d2s_clip(dv(r['x'], dev), scale=case['scale'], shift=case['shift'], clip=case['clip'])
    assert_exact(host(y), r['ref'], case['name'])


@pytest.mark.parametrize('case', params(C.D2S_BWD_CASES))
def test_d2s_clip_bwd(dev, case):
    from neural_imaging_amd import ops
    r = C.d2s_bwd_case(case)
    assert_exact(host(ops.d2s_clip_bwd(dv(r['dy'], dev), scale=case['scale'])), r['ref'], case['name'])


@pytest.mark.parametrize('case', params(C.D2S2_CASES))
def test_d2s2_scale(dev, case):
    from neural_imaging_amd import ops
    r = C.d2s2_case(case)
    assert_exact(host(ops.d2s2_scale(dv(r['xs'], dev), case['c'], scale=case['scale'])), r['ref'], case['name'])


@pytest.mark.parametrize('case', params(C.ZERO_INSERT_CASES))
def test_zero_insert2(dev, case):
    from neural_imaging_amd import ops
    r = C.zero_insert_case(case)
    assert_exact(host(ops.zero_insert2(dv(r['x'], dev))), r['ref'], case['name'])


@pytest.mark.parametrize('case', params(C.CONVT_CASES))
def test_convt2x2_f32(dev, case):
    from neural_imaging_amd import ops
    r = C.convt_case(case)
    if case['mode'] == 'bf16':
        ops.set_compute('bf16')                               # (the autouse fixture of conftest.py returns to float32)
    y = ops.convt2x2(dv(r['x'], dev), dv(r['w'], dev), None if r['b'] is None else dv(r['b'], dev))
    assert y.dtype == torch.float32
    assert_exact(host(y), r['ref'], case['name'])


# ----------------------------------------------------------------------------------------------------------------------
# C. element-wise streams
def _offset_view(a, dev):
    """The array on the device, 4 bytes into its allocation (16-byte alignment lost)."""
    buf = torch.empty(len(a) + 1, device=dev)
    v = buf[1:]
    v.copy_(dv(a, dev))
    assert v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize('count', C.STREAM_COUNTS + [C.PW_BIG, C.PW_BIG + 1], ids=lambda c: 'add_streams-n{}'.format(c))
def test_add_streams(dev, count):
    from neural_imaging_amd import ops
    big = count > 10000
    (a, b), ref2 = C.add_case(count, 2)
    assert_exact(host(ops.add(dv(a, dev), dv(b, dev))), ref2, 'add')
    at = dv(a, dev)
    ops.add(at, dv(b, dev), out=at)
    assert_exact(host(at), ref2, 'add in place')
    for n_in in ((2, 6, 7) if big else range(2, 8)):          # 7: the pairwise fallback; count % 4 != 0: the fallback as well
        xs, ref = C.add_case(count, n_in)
        assert_exact(host(ops.add_n([dv(x, dev) for x in xs])), ref, 'add_n of {}'.format(n_in))
        for j in ((0, n_in - 1) if big else range(n_in)):
            ts = [dv(x, dev) for x in xs]
            out = ops.add_n(ts, out=ts[j])
            assert out is ts[j]
            assert_exact(host(ts[j]), ref, 'add_n of {}, out = input {}'.format(n_in, j))
    if count:
        xs, ref = C.add_case(count, 3)                        # a 4-byte-offset view: the pairwise fallback at any count
        ts = [dv(xs[0], dev), _offset_view(xs[1], dev), dv(xs[2], dev)]
        assert_exact(host(ops.add_n(ts)), ref, 'add_n with an offset input')
        assert_exact(host(ops.add_n(ts, out=ts[1])), ref, 'add_n into the offset input')


@pytest.mark.parametrize('count', C.STREAM_COUNTS + [C.PW_BIG], ids=lambda c: 'simple_streams-n{}'.format(c))
def test_simple_streams(dev, count):
    from neural_imaging_amd import ops
    for alpha in (A, 0.0):
        r = C.lrelu_case(count, alpha)
        assert_exact(host(ops.lrelu_bwd(dv(r['dy'], dev), dv(r['x'], dev), alpha=alpha)), r['bwd'], 'lrelu_bwd alpha {}'.format(alpha))
        assert_exact(host(ops.lrelu(dv(r['x'], dev), alpha=alpha)), r['fwd'], 'lrelu alpha {}'.format(alpha))
    for a, b in ((0.5, 0.5), (0.25, 0.0), (1.0, -0.5)):
        r = C.affine_case(count, a, b)
        assert_exact(host(ops.affine(dv(r['x'], dev), a, b)), r['ref'], 'affine {} {}'.format(a, b))
    assert_exact(host(ops.clip01(dv(r['x'], dev))), r['clip'], 'clip01')
    xt = dv(r['x'], dev)
    ops.clip01(xt, out=xt)
    assert_exact(host(xt), r['clip'], 'clip01 in place')
    ia = np.random.default_rng(count).integers(-2 ** 31, 2 ** 31, size=count, dtype=np.int64).astype(np.int32)
    ib = np.random.default_rng(count + 1).integers(-2 ** 31, 2 ** 31, size=count, dtype=np.int64).astype(np.int32)
    ta, tb = dv(ia, dev, np.int32), dv(ib, dev, np.int32)
    assert ops.int_max_(ta, tb) is ta
    assert np.array_equal(ta.cpu().numpy(), np.maximum(ia, ib)) and np.array_equal(tb.cpu().numpy(), ib)
    ops.int_fill(tb, -7)
    assert np.array_equal(tb.cpu().numpy(), np.full(count, -7, np.int32))
    ops.int_fill(tb)
    assert not tb.any()
    ft = dv(r['x'], dev)
    ops.float_fill(ft, 0.1)
    assert np.array_equal(ft.cpu().numpy(), np.full(count, np.float32(0.1)))


@pytest.mark.parametrize('count', C.STREAM_COUNTS + [C.ISP_BIG], ids=lambda c: 'mask_scale-n{}'.format(c))
def test_mask_scale(dev, count):
    from neural_imaging_amd import ops
    for scale in (2.0, float(np.float32(1 / 0.7))):
        r = C.mask_scale_case(count, scale)
        y = ops.mask_scale(dv(r['x'], dev), dv(r['keep'], dev, np.uint8), scale)
        assert_exact(host(y), r['ref'], 'mask_scale x {}'.format(scale))
    xt = dv(r['x'], dev)
    ops.mask_scale(xt, dv(r['keep'], dev, np.uint8), scale, out=xt)
    assert_exact(host(xt), r['ref'], 'mask_scale in place')


@pytest.mark.parametrize('count', C.STREAM_COUNTS + [C.ISP_BIG], ids=lambda c: 'activation_exact-n{}'.format(c))
def test_activation_exact(dev, count):
    from neural_imaging_amd import ops
    r = C.lrelu_case(count, A)
    for kind, fwd, bwd in (('leaky_relu', r['fwd'], r['bwd']), ('relu', r['relu'], r['relu_bwd'])):
        y = ops.activation(dv(r['x'], dev), kind, alpha=A)
        assert_exact(host(y), fwd, kind)
        # the derivative is taken from the OUTPUT: sign(y) = sign(x) for both kinds (and relu(0) = 0 -> 0)
        assert_exact(host(ops.activation_bwd(dv(r['dy'], dev), y, kind, alpha=A)), bwd, kind + ' backward')
        xt, dt = dv(r['x'], dev), dv(r['dy'], dev)
        assert ops.activation(xt, kind, out=xt, alpha=A) is xt
        assert_exact(host(xt), fwd, kind + ' in place')
        assert ops.activation_bwd(dt, xt, kind, out=dt, alpha=A) is dt
        assert_exact(host(dt), bwd, kind + ' backward in place')


@pytest.mark.parametrize('count', C.STREAM_COUNTS + [C.ISP_BIG], ids=lambda c: 'isp_residual-n{}'.format(c))
def test_isp_residual(dev, count):
    from neural_imaging_amd import ops
    for alpha in (0.25, 0.375):
        for with_f in (True, False):
            for clip in (True, False):
                r = C.residual_case(count, alpha, with_f, clip)
                y = ops.isp_residual(dv(r['x'], dev), None if r['f'] is None else dv(r['f'], dev), dv([alpha], dev), clip=clip)
                assert_exact(host(y), r['ref'], 'alpha {} f {} clip {}'.format(alpha, with_f, clip))


@pytest.mark.parametrize('count', C.RESIDUAL_BWD_COUNTS, ids=lambda c: 'isp_residual_bwd-n{}'.format(c))
def test_isp_residual_bwd(dev, count):
    from neural_imaging_amd import ops
    for alpha in (0.25, 0.375):
        r = C.residual_bwd_case(count, alpha)
        dalpha = torch.full((1,), 7.0, device=dev)
        df = ops.isp_residual_bwd(dv(r['dy'], dev), dv(r['f'], dev), dv([alpha], dev), dalpha)
        assert_exact(host(df), r['df'], 'df')
        assert_exact(host(dalpha), [r['dalpha']], 'dalpha')       # (the empty call zeroes it)
        r2 = C.residual_bwd_case(count, alpha, existing=-12.0)
        dalpha = torch.full((1,), -12.0, device=dev)
        ops.isp_residual_bwd(dv(r['dy'], dev), dv(r['f'], dev), dv([alpha], dev), dalpha, accumulate=True)
        assert_exact(host(dalpha), [r2['dalpha']], 'dalpha accumulated')       # (the empty call leaves it)


@pytest.mark.parametrize('case', params(C.CONSTRAINED_CASES))
def test_constrained_kernel_exact(dev, case):
    from neural_imaging_amd import ops
    r = C.constrained_case(case)
    k = dv(r['k'], dev)
    assert_exact(host(ops.constrained_kernel(k, strength=case['strength'])), r['nf'], 'normalised filter')
    dk = torch.full_like(k, 7.0)
    ops.constrained_kernel_bwd(k, dv(r['dnf'], dev), dk, strength=case['strength'])
    assert_exact(host(dk), r['dk'], 'kernel gradient')


def test_constrained_refuses_17(dev):
    from neural_imaging_amd import ops
    k = torch.ones((3, 3, 17, 17), device=dev)
    with pytest.raises(RuntimeError):
        ops.constrained_kernel(k)
    with pytest.raises(RuntimeError):
        ops.constrained_kernel_bwd(k, k.clone(), torch.empty_like(k))


@pytest.mark.parametrize('ks,c', [(3, 16), (5, 3), (7, 1)])
def test_constrained_random_float(dev, ks, c):
    """One random float case per size at the tolerance of tests/test_gpu_ops.py::test_constrained_conv."""
    from neural_imaging_amd import ops
    rng = np.random.default_rng(ks * 100 + c)
    k = (rng.uniform(0.2, 1.0, size=(ks, ks, c, c))).astype(np.float32)
    dnf = rng.uniform(-1, 1, size=k.shape).astype(np.float32)
    nf, dkref = C.constrained_reference(k, dnf, 100.0)
    kg = dv(k, dev)
    assert_close(host(ops.constrained_kernel(kg)), nf, 1e-4, 1e-6, what='normalised filter')
    dk = torch.empty_like(kg)
    ops.constrained_kernel_bwd(kg, dv(dnf, dev), dk)
    assert_close(host(dk), dkref, 1e-4, 1e-4, what='constrained kernel grad')


@pytest.mark.parametrize('case', params(C.CONFUSION_CASES))
def test_confusion_accumulate(dev, case):
    from neural_imaging_amd import ops
    r = C.confusion_case(case)
    k = case['k']
    probs, labels = dv(r['probs'], dev), dv(r['labels'], dev, np.int32)
    conf = torch.zeros((k, k), dtype=torch.int64, device=dev)
    pred = ops.confusion_accumulate(probs, labels, conf)
    assert np.array_equal(pred.cpu().numpy(), r['pred']) and np.array_equal(conf.cpu().numpy(), r['conf'])
    assert ops.confusion_accumulate(probs, labels, conf, want_pred=False) is None             # conf alone; the second call accumulates
    assert np.array_equal(conf.cpu().numpy(), 2 * r['conf'])
    assert np.array_equal(ops.confusion_accumulate(probs).cpu().numpy(), r['pred'])           # pred alone
    assert np.array_equal(conf.cpu().numpy(), 2 * r['conf'])


@pytest.mark.parametrize('count', C.STREAM_COUNTS + [C.PW_BIG], ids=lambda c: 'transcendental-n{}'.format(c))
def test_transcendental_streams(dev, count):
    """expf / tanhf / powf kinds at the tolerances of test_classic_isp_pointwise (values 1e-6, gamma 2e-6, derivatives 1e-5)."""
    from neural_imaging_amd import ops
    rng = np.random.default_rng(count + 17)
    x = rng.uniform(-3, 3, size=count).astype(np.float32)
    dy = rng.uniform(-1, 1, size=count).astype(np.float32)
    x64, dy64 = to64(x), to64(dy)
    refs = {'tanh': torch.tanh(x64), 'sigmoid': torch.sigmoid(x64), 'softsign': x64 / (1 + x64.abs())}
    ders = {'tanh': 1 - refs['tanh'] ** 2, 'sigmoid': refs['sigmoid'] * (1 - refs['sigmoid']), 'softsign': 1 / (1 + x64.abs()) ** 2}
    for kind in ('tanh', 'sigmoid', 'softsign'):
        y = ops.activation(dv(x, dev), kind)
        assert_close(host(y), refs[kind].numpy(), 1e-6, what='activation ' + kind)
        assert_close(host(ops.activation_bwd(dv(dy, dev), y, kind)), (dy64 * ders[kind]).numpy(), 1e-5, what='activation_bwd ' + kind)
    y = ops.tanh(dv(x, dev))
    assert_close(host(y), refs['tanh'].numpy(), 1e-6, what='tanh')
    assert_close(host(ops.tanh_bwd(dv(dy, dev), y)), (dy64 * ders['tanh']).numpy(), 1e-5, what='tanh_bwd')
    y = ops.sigmoid(dv(x, dev))
    assert_close(host(y), refs['sigmoid'].numpy(), 1e-6, what='sigmoid')
    assert_close(host(ops.sigmoid_bwd(dv(dy, dev), y)), (dy64 * ders['sigmoid']).numpy(), 1e-5, what='sigmoid_bwd')
    v = rng.uniform(-0.3, 1.4, size=count).astype(np.float32)
    vc = torch.clamp(to64(v), 1.0 / 255, 1.0)
    assert_close(host(ops.gamma_ste(dv(v, dev))), (vc ** (1 / 2.2)).numpy(), 2e-6, what='gamma')
    assert_close(host(ops.gamma_ste_bwd(dv(v, dev), dv(dy, dev))), (dy64 * (1 / 2.2) * vc ** (1 / 2.2 - 1)).numpy(), 1e-5, what='d gamma')


def test_saturated_ends(dev):
    from neural_imaging_amd import ops
    x = dv([100.0, -100.0, 20.0, -20.0], dev)
    assert host(ops.sigmoid(x))[:2].tolist() == [1.0, 0.0]
    assert host(ops.activation(x, 'sigmoid'))[:2].tolist() == [1.0, 0.0]
    assert host(ops.tanh(x))[2:].tolist() == [1.0, -1.0]
    assert host(ops.activation(x, 'tanh'))[2:].tolist() == [1.0, -1.0]
    lo, hi, e = 1.0 / 255, 1.0, 1.0 / 2.2
    v = dv([-0.5, lo, hi, 1.5, 0.0], dev)
    gy = host(ops.gamma_ste(v))
    low = float(np.float32(lo)) ** e
    assert gy[2] == 1.0 and gy[3] == 1.0 and gy[0] == gy[1] == gy[4] and abs(gy[1] - low) <= 2e-6
    gd = host(ops.gamma_ste_bwd(v, torch.ones_like(v)))        # straight-through: the clipped value's slope everywhere
    assert gd[2] == gd[3] and abs(gd[2] - e) <= 1e-6 and gd[0] == gd[1] == gd[4] and abs(gd[1] - e * float(np.float32(lo)) ** (e - 1)) <= 1e-5


# ----------------------------------------------------------------------------------------------------------------------
# D. SSIM family
@pytest.mark.parametrize('case', params(C.SSIM_CASES))
def test_ssim(dev, case):
    from neural_imaging_amd import ops
    r = C.ssim_case(case)
    a, b = dv(r['a'], dev), dv(r['b'], dev)
    got = host(ops.ssim(a, b, mode=case['mode']))
    print('{}: max |ssim - ref| {:.3e}'.format(case['name'], np.abs(got - r['ref']).max()))
    assert np.abs(got - r['ref']).max() <= 1e-5
    got255 = host(ops.ssim(a * 255.0, b * 255.0, mode=case['mode'], max_val=255.0))
    assert np.abs(got255 - r['ref']).max() <= 1e-5, 'ssim(255 a, 255 b, max_val = 255)'
    same = host(ops.ssim(a, a, mode=case['mode']))
    assert (same == 1.0).all(), 'ssim(a, a) = {!r}'.format(same.tolist())


@pytest.mark.parametrize('mode,max_val', [('skimage', 1.0), ('skimage', 255.0), ('tf', 1.0), ('tf', 255.0)])
def test_ssim_constant_images(dev, mode, max_val):
    from neural_imaging_amd import ops
    p, q = 0.25, 0.625
    shape = (2, 23, 29, 3)
    a = torch.full(shape, p * max_val, device=dev)
    b = torch.full(shape, q * max_val, device=dev)
    c1 = (0.01 * max_val) ** 2
    want = (2 * p * q * max_val ** 2 + c1) / ((p * p + q * q) * max_val ** 2 + c1)
    got = host(ops.ssim(a, b, mode=mode, max_val=max_val))
    assert np.abs(got - want).max() <= 1e-7, (got.tolist(), want)


def _loss_close(got, ref):
    assert abs(got - ref) <= 2e-6 * max(1.0, abs(ref)), (got, ref)          # (the bound of test_image_losses_with_gradient)


@pytest.mark.parametrize('case', params(C.SSIM_LOSS_CASES))
def test_ssim_loss(dev, case):
    from neural_imaging_amd import ops
    r = C.ssim_loss_case(case)
    y, t, mv = dv(r['y'], dev), dv(r['t'], dev), case['max_val']
    loss, grad = ops.ssim_loss(y, t, grad_scale=1.0, max_val=mv)
    print('{}: loss {!r} (reference {!r})'.format(case['name'], float(loss.item()), float(r['loss'])))
    _loss_close(float(loss.item()), float(r['loss']))
    assert_close(host(grad), r['grad'], 1e-7, 1e-5, what='SSIM gradient')
    acc = dv(r['base'], dev)
    loss2, out = ops.ssim_loss(y, t, grad_scale=0.25, grad_out=acc, accumulate=True, max_val=mv)
    assert out is acc and float(loss2.item()) == float(loss.item())
    assert_close(host(acc), r['acc'], 1e-6, 1e-5, what='SSIM accumulated gradient')
    loss3, none = ops.ssim_loss(y, t, max_val=mv)
    assert none is None and float(loss3.item()) == float(loss.item())


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev)


def _p(t):
    return None if t is None else t.data_ptr()


@pytest.mark.parametrize('case', params(C.PLANES_CASES))
def test_ssim_planes(dev, case):
    from neural_imaging_amd import _lib, ops
    r = C.planes_case(case)
    n, h, w, c, which = case['n'], case['h'], case['w'], case['c'], case['which']
    y, t = dv(r['y'], dev), dv(r['t'], dev)
    ms = torch.full((n, c), 7.0, device=dev) if case['out'] in ('both', 'ssim') else None
    mcs = torch.full((n, c), 7.0, device=dev) if case['out'] in ('both', 'cs') else None
    maps = torch.full((3, n, h - 10, w - 10, c), 7.0, device=dev) if which else None
    ws = _ws(_lib.load().nimg_ssim_planes_workspace_bytes(n, c), dev)
    _lib.call('nimg_ssim_planes', _p(y), _p(t), n, h, w, c, 1.0, _p(ops._ssim_window(dev)), _p(ms), _p(mcs), _p(maps), which, _p(ws),
              ws.numel(), ops._stream())
    if ms is not None:
        assert np.abs(host(ms) - r['mean_ssim']).max() <= 1e-5
    if mcs is not None:
        assert np.abs(host(mcs) - r['mean_cs']).max() <= 1e-5
    if which:
        d = np.abs(host(maps).astype(np.float64) - r['maps'])
        worst = float((d / C.maps_bound(r['maps'])).max())
        print('{}: worst map error / bound {:.3f}'.format(case['name'], worst))
        assert worst <= 1.0, 'derivative maps off by {:.3f} x (2^-23 |ref| + 1e-12)'.format(worst)


@pytest.mark.parametrize('planes', C.COMBINE_PLANES, ids=lambda p: 'msssim_combine-p{}'.format(p))
@pytest.mark.parametrize('with_coef', [True, False], ids=['coef', 'nocoef'])
def test_msssim_combine(dev, planes, with_coef):
    from neural_imaging_amd import _lib, ops
    r = C.combine_case(planes)
    loss = torch.full((1,), 7.0, device=dev)
    coef = torch.full((5, planes), 7.0, device=dev) if with_coef else None
    values, items = dv(r['values'], dev), dv(r['items'], dev)
    _lib.call('nimg_msssim_combine', _p(values), _p(items), 5, planes, _p(loss), _p(coef), ops._stream())
    assert abs(float(loss.item()) - r['loss']) <= 1e-6 * abs(r['loss'])
    if with_coef:
        got = host(coef).astype(np.float64)
        assert (np.abs(got - r['coef']) <= 1e-6 * np.abs(r['coef'])).all()
        assert (got[r['values'] <= 0] == 0).all()


def test_ssim_maps_grad(dev):
    from neural_imaging_amd import _lib, ops
    r = C.maps_grad_case()
    n, h, w, c = r['y'].shape
    y, t, maps, coef = dv(r['y'], dev), dv(r['t'], dev), dv(r['maps'], dev), dv(r['coef'], dev)
    for acc in (False, True):
        g = dv(r['base'], dev)
        _lib.call('nimg_ssim_maps_grad', _p(y), _p(t), _p(maps), _p(coef), _p(g), n, h, w, c,
                  _p(ops._ssim_window(dev)), 0.5, 1 if acc else 0, ops._stream())
        assert_close(host(g), r['acc'] if acc else r['ref'], 1e-7, 1e-5, what='maps gradient, accumulate {}'.format(acc))


def test_msssim_end_to_end(dev):
    from neural_imaging_amd import ops
    from oracle import tfops as T
    y, t = C.image_pair(1, 176, 192, 2, 41)
    yt = to64(y).requires_grad_(True)
    ref = T.msssim_loss255(yt, to64(t))
    gref, = torch.autograd.grad(ref, [yt])
    loss, grad = ops.msssim_loss(dv(y, dev), dv(t, dev), grad_scale=1.0)
    _loss_close(float(loss.item()), float(ref.detach()))
    assert_close(host(grad), gref.numpy(), 1e-7, 1e-5, what='MS-SSIM gradient')
