"""
Parity tests proper: every HIP entry point (called through the C ABI via neural_imaging_amd.ops) against the CPU oracle
on identical seeded inputs.  float tolerance: 1e-4 absolute on [0,1]-scaled activations (north_star), and for gradient
tensors max-abs-error <= 1e-4 x max|reference| ; the JPEG quantisation index tensor is compared with ==.
"""
import numpy as np
import pytest
import torch

from oracle import djpeg as odj
from oracle import manip as om
from oracle import tables as ot
from oracle import tfops as T

from util import assert_close, natural_images, to64

pytestmark = pytest.mark.gpu

ATOL = 1e-4
GRTOL = 1e-4


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    return torch.device('cuda', 0)


def g(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev).contiguous()


def rnd(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# dJPEG
@pytest.mark.parametrize('shape,q', [((2, 64, 64), 50), ((1, 8, 8), 80), ((3, 40, 72), 10), ((2, 128, 256), 95),
                                      ((1, 512, 512), 50)])
def test_djpeg_fwd_bit_exact_index_path(dev, shape, q):
    from neural_imaging_amd import ops
    from test_oracle import c_djpeg
    n, h, w = shape
    x = natural_images(n, h, w, seed=q + h)
    if h == 40:
        x = np.random.default_rng(5).random((n, h, w, 3)).astype(np.float32)     # pure noise: worst case for ties
    yc, idxc, xdc = c_djpeg(x, q)
    y, mask, idx, xdq = ops.djpeg_fwd(g(x, dev), ops.qtables_device(q, dev), 'soft', want_idx=True, want_xdq=True)
    assert torch.equal(idx.cpu(), torch.from_numpy(idxc)), 'quantisation indices differ from the canonical-order oracle'
    assert np.array_equal(xdq.cpu().numpy(), xdc)
    assert np.abs(y.cpu().numpy() - yc).max() <= 1e-6
    # against float64 the hard rounding can flip where |X/Q - (k + 1/2)| is below float32 resolution: a flipped index
    # moves a whole block by one quantisation step, so compare statistically there and tightly everywhere else
    y64, _, idx64 = odj.djpeg_torch(to64(x), q, 'soft')
    flips = (idx.cpu().numpy() != idx64.numpy())
    assert flips.mean() < 1e-4, flips.mean()
    blk_ok = ~flips.any(axis=(1, 4, 5))                                        # (n, hb, wb) blocks without a flip
    d = np.abs(y.cpu().numpy() - y64.numpy()).reshape(n, h // 8, 8, w // 8, 8, 3).max(axis=(2, 4, 5))
    assert d[blk_ok].max() <= ATOL, d[blk_ok].max()
    # mask = "not clipped"
    ypre_in = (y64.numpy() > 0) & (y64.numpy() < 1)
    m = mask.cpu().numpy()
    bits = np.stack([(m >> c) & 1 for c in range(3)], axis=-1).astype(bool)
    assert (bits[ypre_in]).mean() > 0.999


@pytest.mark.parametrize('mode', ['soft', 'sin', 'harmonic', 'identity'])
def test_djpeg_modes_fwd_bwd(dev, mode):
    from neural_imaging_amd import ops
    x = natural_images(2, 32, 48, seed=11)
    gy = rnd(x.shape, 12)
    qn = np.stack([ot.jpeg_qtable(50, 0), ot.jpeg_qtable(50, 1), ot.jpeg_qtable(50, 1)]).astype(np.float64)
    yn, cache = odj.djpeg_numpy_fwd(x, qn, mode)
    gn = odj.djpeg_numpy_bwd(gy.astype(np.float64), cache)
    q = ops.qtables_device(50, dev)
    y, mask, _, _ = ops.djpeg_fwd(g(x, dev), q, mode)
    assert_close(y.cpu().numpy(), yn, ATOL, what='djpeg fwd ' + mode)
    gx = ops.djpeg_bwd(g(x, dev), g(gy, dev), mask, q, mode)
    assert_close(gx.cpu().numpy(), gn, 1e-5, GRTOL * 3, what='djpeg bwd ' + mode)


@pytest.mark.parametrize('mode', ['soft', 'sin', 'harmonic'])
def test_djpeg_trainable_tables(dev, mode):
    """DifferentiableJPEG(trainable=True) (models/jpeg.py:57-62): the two (8,8) weights Q_mtx_luma / Q_mtx_chroma feed the kernel
    ([Y, Cb, Cr] = [luma, chroma, chroma], :125-128) and receive their gradient through X / Q -> quant -> * Q (:129-131) from
    nimg_djpeg_bwd_dq; oracle = autograd of oracle/djpeg.py in float64 with the tables as leaves.  Also the explicit-quality
    swap (a numeric quality passed to forward uses that quality's constant tables, :235-243) and accumulation."""
    from neural_imaging_amd.models import jpeg as mj
    x = natural_images(3, 32, 48, seed=21)
    gy = rnd(x.shape, 22)
    rng = np.random.default_rng(23)
    ql = (ot.jpeg_qtable(60, 0) * rng.uniform(0.7, 1.3, (8, 8))).astype(np.float32)       # non-integer: they are weights now
    qc = (ot.jpeg_qtable(60, 1) * rng.uniform(0.7, 1.3, (8, 8))).astype(np.float32)
    tl, tc = to64(ql).requires_grad_(True), to64(qc).requires_grad_(True)
    xt = to64(x).requires_grad_(True)
    y_ref, _, _ = odj.djpeg_torch(xt, mode=mode, q=torch.stack([tl, tc, tc]))
    (y_ref * to64(gy)).sum().backward()
    codec = mj.JPEG(quality=60, codec=mode, trainable=True, device=dev)
    assert codec.parameter_names == ['Q_mtx_luma', 'Q_mtx_chroma'] and codec.count_parameters() == 128
    assert np.array_equal(codec.state_dict()['Q_mtx_chroma'], ot.jpeg_qtable(60, 1).astype(np.float32))     # initialiser
    codec.load_state_dict({'Q_mtx_luma': ql, 'Q_mtx_chroma': qc})
    y, ctx = codec.forward(g(x, dev), training=True)
    assert_close(y.cpu().numpy(), y_ref.detach().numpy(), ATOL, what='fwd with trained tables')
    gx = codec.backward(ctx, g(gy, dev))
    assert_close(gx.cpu().numpy(), xt.grad.numpy(), 1e-5, GRTOL * 3, what='d/dx')
    dq = codec._model.flat_grad.view(2, 8, 8).cpu().numpy()
    assert_close(dq[0], tl.grad.numpy(), 1e-6, GRTOL * 3, what='d/dQ luma')
    assert_close(dq[1], tc.grad.numpy(), 1e-6, GRTOL * 3, what='d/dQ chroma')
    codec.backward(ctx, g(gy, dev), accumulate=True)
    assert_close(codec._model.flat_grad.view(2, 8, 8).cpu().numpy(), 2 * dq, 1e-6, 1e-5, what='accumulate')
    # an explicit quality bypasses the weights (and leaves their gradients alone)
    y80, ctx80 = codec.forward(g(x, dev), quality=80, training=True)
    plain = mj.JPEG(quality=80, codec=mode, device=dev)
    assert torch.equal(y80, plain.forward(g(x, dev))[0])
    before = codec._model.flat_grad.clone()
    codec.backward(ctx80, g(gy, dev))
    assert torch.equal(before, codec._model.flat_grad)
    # ... but an explicit quality EQUAL to the constructor's keeps the learned tables (the reference swaps only when the
    # resolved quality differs, models/jpeg.py:235-243)
    y60, ctx60 = codec.forward(g(x, dev), quality=60, training=True)
    assert ctx60['learned'] and torch.equal(y60, y)
    assert not torch.equal(y60, mj.JPEG(quality=60, codec=mode, device=dev).forward(g(x, dev))[0])
    with pytest.raises(ValueError):                                        # unspecified quality: raises before any table is picked
        mj.JPEG(quality=None, codec=mode, trainable=True, device=dev).forward(g(x, dev))


def test_djpeg_properties_full_size(dev):
    """BASELINE size (batch of 256x256): size-independent properties instead of the (slow) oracle."""
    from neural_imaging_amd import ops
    x = g(natural_images(8, 256, 256, seed=2), dev)
    q = ops.qtables_device(80, dev)
    y, mask, idx, xdq = ops.djpeg_fwd(x, q, 'soft', want_idx=True, want_xdq=True)
    assert float(y.min()) >= 0 and float(y.max()) <= 1
    # dequantised coefficients are exact multiples of the table; indices are what the table divides them into
    qb = q.reshape(1, 3, 1, 1, 8, 8)
    assert torch.equal(idx.float() * qb, xdq)
    # idempotence of the index path under a translation by whole blocks
    y2, _, idx2, _ = ops.djpeg_fwd(torch.roll(x, shifts=(8, 16), dims=(1, 2)).contiguous(), q, 'soft', want_idx=True)
    assert torch.equal(torch.roll(idx, shifts=(1, 2), dims=(2, 3)), idx2)
    # PSNR sanity vs input
    psnr = 10 * torch.log10(1.0 / ((y - x) ** 2).mean())
    assert 28 < float(psnr) < 50


# ------------------------------------------------------------------------------------------------------------------
# convolutions
CONV_CASES = [
    # n, h, w, c1, c2, cout, ks, stride, act
    (2, 16, 16, 4, 0, 32, 3, 1, 'leaky_relu'),
    (2, 16, 16, 32, 0, 32, 3, 1, 'leaky_relu'),
    (2, 32, 32, 16, 16, 32, 3, 1, 'leaky_relu'),
    (2, 20, 24, 8, 0, 12, 3, 1, None),
    (2, 32, 32, 3, 0, 32, 5, 1, 'leaky_relu'),
    (2, 32, 32, 32, 0, 64, 5, 1, 'leaky_relu'),
    (5, 8, 8, 64, 0, 64, 1, 1, 'leaky_relu'),
    (6, 8, 8, 64, 0, 128, 3, 1, 'leaky_relu'),
    (3, 16, 16, 48, 0, 96, 3, 1, None),
    (2, 32, 32, 3, 0, 64, 5, 2, 'leaky_relu'),
    (2, 32, 32, 64, 0, 128, 5, 2, None),
    (1, 64, 64, 40, 0, 72, 5, 1, 'leaky_relu'),
    (2, 40, 72, 3, 0, 32, 5, 1, 'leaky_relu'),      # packed (tap,ci) reduction, partial tiles
    (2, 24, 24, 4, 0, 64, 3, 1, None),
    (3, 32, 80, 32, 0, 3, 5, 1, None),              # few-output VALU kernel (FAN conv1 dgrad shape)
    (2, 20, 36, 3, 0, 3, 5, 1, None),
    (2, 16, 16, 16, 0, 3, 3, 1, None),
]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv2d_fwd(dev, case):
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout, ks, stride, act = case
    x1, x2 = rnd((n, h, w, c1), 1), (rnd((n, h, w, c2), 2) if c2 else None)
    wt = rnd((ks, ks, c1 + c2, cout), 3, -0.2, 0.2)
    b = rnd((cout,), 4)
    xin = to64(x1) if x2 is None else torch.cat([to64(x1), to64(x2)], dim=-1)
    ref = T.conv2d(xin, to64(wt), to64(b), stride, 'SAME')
    if act:
        ref = T.leaky_relu(ref)
    out = ops.conv2d(g(x1, dev), g(wt, dev), g(b, dev), x2=None if x2 is None else g(x2, dev), stride=stride, act=act)
    assert tuple(out.shape) == tuple(ref.shape)
    assert_close(out.cpu().numpy(), ref.numpy(), ATOL, GRTOL, what='conv fwd {}'.format(case))


@pytest.mark.parametrize('case', [c for c in CONV_CASES if c[7] == 1])
def test_conv2d_dgrad_wgrad(dev, case):
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout, ks, stride, act = case
    x = to64(rnd((n, h, w, c1 + c2), 1)).requires_grad_(True)
    wt = to64(rnd((ks, ks, c1 + c2, cout), 3, -0.2, 0.2)).requires_grad_(True)
    b = to64(rnd((cout,), 4)).requires_grad_(True)
    dz = rnd((n, h, w, cout), 5)
    prev_act = rnd((n, h, w, c1 + c2), 6)           # saved activation of the previous layer (for the fused lrelu')
    z = T.conv2d(x, wt, b, 1, 'SAME')
    (z * to64(dz)).sum().backward()
    # weight / bias gradients
    xg = g(x.detach().numpy(), dev)
    dbf = torch.empty((cout,), device=dev)
    if c2:
        dw = ops.conv2d_wgrad(xg[..., :c1].contiguous(), g(dz, dev), ks, x2=xg[..., c1:].contiguous(), db=dbf)
    else:
        dw = ops.conv2d_wgrad(xg, g(dz, dev), ks, db=dbf)
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 1e-5, GRTOL, what='wgrad {}'.format(case))
    assert_close(dbf.cpu().numpy(), b.grad.numpy(), 1e-5, GRTOL, what='fused bias grad {}'.format(case))
    db = ops.bias_grad(g(dz, dev))
    assert_close(db.cpu().numpy(), b.grad.numpy(), 1e-5, GRTOL, what='bias grad {}'.format(case))
    # input gradient, with the previous layer's LeakyReLU derivative fused
    mask = np.where(prev_act > 0, 1.0, 0.2)
    if c2:
        o1 = torch.empty((n, h, w, c1), device=dev)
        o2 = torch.empty((n, h, w, c2), device=dev)
        ops.conv2d_dgrad(g(dz, dev), g(wt.detach().numpy(), dev), (h, w), out=o1, out2=o2)
        dx = torch.cat([o1, o2], dim=-1)
        assert_close(dx.cpu().numpy(), x.grad.numpy(), 1e-5, GRTOL, what='dgrad(2 outputs) {}'.format(case))
    else:
        dx = ops.conv2d_dgrad(g(dz, dev), g(wt.detach().numpy(), dev), (h, w), act_mask=g(prev_act, dev))
        assert_close(dx.cpu().numpy(), x.grad.numpy() * mask, 1e-5, GRTOL, what='dgrad {}'.format(case))


def test_conv2d_strided_wgrad(dev):
    from neural_imaging_amd import ops
    n, h, w, cin, cout, ks = 2, 32, 32, 16, 32, 5
    x = to64(rnd((n, h, w, cin), 1))
    wt = to64(rnd((ks, ks, cin, cout), 3, -0.2, 0.2)).requires_grad_(True)
    z = T.conv2d(x, wt, None, 2, 'SAME')
    dz = rnd(tuple(z.shape), 5)
    (z * to64(dz)).sum().backward()
    dw = ops.conv2d_wgrad(g(x.numpy(), dev), g(dz, dev), ks, stride=2)
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 1e-5, GRTOL, what='strided wgrad')


def test_convt2x2_fwd_bwd(dev):
    from neural_imaging_amd import ops
    n, h, w, cin, cout = 2, 8, 12, 64, 32
    x = to64(rnd((n, h, w, cin), 1)).requires_grad_(True)
    wt = to64(rnd((2, 2, cout, cin), 2, -0.3, 0.3)).requires_grad_(True)
    b = to64(rnd((cout,), 3)).requires_grad_(True)
    y = T.conv2d_transpose_2x2(x, wt, b)
    dy = rnd(tuple(y.shape), 4)
    (y * to64(dy)).sum().backward()
    yo = ops.convt2x2(g(x.detach().numpy(), dev), g(wt.detach().numpy(), dev), g(b.detach().numpy(), dev))
    assert_close(yo.cpu().numpy(), y.detach().numpy(), ATOL, GRTOL, what='convT fwd')
    prev = rnd((n, h, w, cin), 9)
    dx = ops.convt2x2_dgrad(g(dy, dev), g(wt.detach().numpy(), dev), act_mask=g(prev, dev))
    assert_close(dx.cpu().numpy(), x.grad.numpy() * np.where(prev > 0, 1.0, 0.2), 1e-5, GRTOL, what='convT dgrad')
    dw = ops.convt2x2_wgrad(g(x.detach().numpy(), dev), g(dy, dev))
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 1e-5, GRTOL, what='convT wgrad')
    db = ops.bias_grad(g(dy, dev))
    assert_close(db.cpu().numpy(), b.grad.numpy(), 1e-5, GRTOL, what='convT bias grad')


# ------------------------------------------------------------------------------------------------------------------
# pooling / layout / element-wise
@pytest.mark.parametrize('c', [3, 32])
def test_maxpool_fwd_bwd_with_ties(dev, c):
    from neural_imaging_amd import ops
    n, h, w = 2, 8, 12
    x = np.round(rnd((n, h, w, c), 1) * 4) / 4            # coarse values => many exact ties
    xt = to64(x).requires_grad_(True)
    y = T.max_pool2(xt)
    dp = rnd(tuple(y.shape), 2)
    (y * to64(dp)).sum().backward()
    yo = ops.maxpool2(g(x, dev))
    assert np.array_equal(yo.cpu().numpy(), y.detach().numpy().astype(np.float32))
    add = rnd((n, h, w, c), 3)
    dz = ops.maxpool2_bwd(g(dp, dev), g(x, dev), add=g(add, dev), apply_mask=True)
    ref = (xt.grad.numpy() + add) * np.where(x > 0, 1.0, 0.2)
    assert_close(dz.cpu().numpy(), ref, 1e-6, what='maxpool bwd (first-max tie rule)')


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('cin,cout,ks,h,w', [(3, 32, 5, 32, 48), (32, 64, 5, 32, 32), (16, 24, 3, 16, 16),
                                              (64, 128, 5, 20, 28), (4, 64, 3, 18, 34), (8, 256, 5, 6, 10)])
def test_conv_pool_fused_epilogue(dev, mode, cin, cout, ks, h, w):
    """conv -> LeakyReLU -> MaxPool2D fused in the convolution epilogue == the three separate passes, bit for bit
    (same accumulation, same first-maximum tie rule), and its arg-max bytes reproduce the un-fused backward."""
    from neural_imaging_amd import ops
    n = 3
    x, wt, b = rnd((n, h, w, cin), 1), rnd((ks, ks, cin, cout), 2, -0.2, 0.2), rnd((cout,), 3, -0.1, 0.1)
    ops.set_compute(mode)
    try:
        for wv in (wt, np.zeros_like(wt)):                      # zero weights: every window is a 4-way tie
            xd, wd, bd = g(x, dev), g(wv, dev), g(b, dev)
            full = ops.conv2d(xd, wd, bd, act='leaky_relu')
            pooled_ref = ops.maxpool2(full)
            pooled, idx = ops.conv2d_pool(xd, wd, bd, act='leaky_relu')
            assert np.array_equal(pooled.cpu().numpy(), pooled_ref.cpu().numpy())
            assert int(idx.max()) <= 3
            dp = g(rnd(tuple(pooled.shape), 4), dev)
            dz_ref = ops.maxpool2_bwd(dp, full, None, apply_mask=True)
            dz = ops.maxpool2_unpool(dp, idx, pooled, apply_mask=True)
            assert np.array_equal(dz.cpu().numpy(), dz_ref.cpu().numpy())
    finally:
        ops.set_compute('f32')


@pytest.mark.parametrize('n,cin,cout,h,w', [(3, 32, 32, 128, 128), (3, 64, 64, 64, 64), (5, 128, 128, 32, 32), (5, 256, 256, 16, 16),
                                            (2, 16, 24, 24, 40), (1, 8, 72, 10, 18)])
def test_conv_writes_activation_and_pooled_tensor(dev, n, cin, cout, h, w):
    """The UNet encoder's second convolutions store the skip tensor AND its max-pool from one epilogue (ops.conv2d_and_pool):
    both equal the two separate passes bit for bit - the generic and the LDS-DMA 3x3 kernels, ragged tiles, ragged channels."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    try:
        x = g(rnd((n, h, w, cin), 1), dev).to(torch.bfloat16)
        wt, b = g(rnd((3, 3, cin, cout), 2, -0.2, 0.2), dev), g(rnd((cout,), 3, -0.1, 0.1), dev)
        assert ops.conv2d_and_pool_ok(x, wt)
        for act in ('leaky_relu', None):
            full = ops.conv2d(x, wt, b, act=act, out_bf16=True)
            y, pooled = ops.conv2d_and_pool(x, wt, b, act=act)
            assert y.dtype == torch.bfloat16 and pooled.dtype == torch.bfloat16
            assert torch.equal(y, full)
            assert torch.equal(pooled, ops.maxpool2(full))
        assert not ops.conv2d_and_pool_ok(x[:, :8, :8], wt)          # 8 x 8 images take the four-image tiles: separate passes
        with pytest.raises(ValueError):
            ops.conv2d_and_pool(x[:, :8, :8].contiguous(), wt, b)
    finally:
        ops.set_compute('f32')


@pytest.mark.parametrize('n,cin,cout,h,w', [(3, 32, 64, 64, 64), (3, 64, 128, 32, 32), (5, 128, 256, 16, 16), (5, 256, 512, 8, 8),
                                            (2, 16, 24, 12, 20), (1, 8, 72, 6, 10)])
@pytest.mark.parametrize('with_skip', [True, False])
def test_input_gradient_written_through_the_max_pool(dev, n, cin, cout, h, w, with_skip):
    """ops.conv2d_dgrad_unpool_out = conv2d_dgrad (stored as bf16) -> maxpool2_bwd (route to the first maximum + skip gradient +
    LeakyReLU') in the convolution's epilogue: bit-identical, in place on the skip buffer, for the generic and the LDS-DMA
    kernels, the four-image 8 x 8 tiles and ragged shapes."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    try:
        bf = torch.bfloat16
        dz = g(rnd((n, h, w, cout), 1), dev).to(bf)
        wt = g(rnd((3, 3, cin, cout), 2, -0.2, 0.2), dev)
        act = (torch.round(g(rnd((n, 2 * h, 2 * w, cin), 3), dev) * 4) / 4).to(bf)        # coarse values: ties inside the windows
        skip = g(rnd((n, 2 * h, 2 * w, cin), 4), dev).to(bf) if with_skip else None
        assert ops.conv2d_dgrad_unpool_out_ok(dz, wt, act, skip)
        for mask in (True, False):
            d_pool = ops.conv2d_dgrad(dz, wt, (h, w), out_bf16=True)
            ref = ops.maxpool2_bwd(d_pool, act, add=skip, apply_mask=mask)
            out = ops.conv2d_dgrad_unpool_out(dz, wt, act, skip=skip, apply_mask=mask)
            assert out.dtype == bf and torch.equal(out, ref)
        if with_skip:
            buf = skip.clone()
            res = ops.conv2d_dgrad_unpool_out(dz, wt, act, skip=buf, apply_mask=True, out=buf)
            assert res.data_ptr() == buf.data_ptr() and torch.equal(buf, ops.maxpool2_bwd(d_pool, act, add=skip, apply_mask=True))
    finally:
        ops.set_compute('f32')


@pytest.mark.parametrize('n_parts', [1, 2, 5, 6])
def test_head_gradient_in_one_pass(dev, n_parts):
    """ops.mse255_sum_s2d3 = add_n -> mse255(accumulate) -> d2s_clip_bwd(scale 1) in one pass: the same additions in the same
    order (bit-identical gradient), the loss to float32 rounding of its float64 sum."""
    from neural_imaging_amd import ops
    n, h2, w2 = 3, 24, 40
    parts = [g(rnd((n, h2, w2, 3), 10 + k, -0.1, 0.1), dev) for k in range(n_parts)]
    y, t = g(rnd((n, h2, w2, 3), 1, 0, 1), dev), g(rnd((n, h2, w2, 3), 2, 0, 1), dev)
    s = ops.add_n(parts) if n_parts > 1 else parts[0].clone()
    loss_ref, _ = ops.mse255(y, t, grad_scale=0.1, grad_out=s, accumulate=True)
    dz_ref = ops.d2s_clip_bwd(s, 1.0)
    loss, dz = ops.mse255_sum_s2d3(parts, y, t, 0.1)
    assert dz.shape == (n, h2 // 2, w2 // 2, 12) and torch.equal(dz, dz_ref)
    assert abs(float(loss) - float(loss_ref)) <= 1e-6 * abs(float(loss_ref))
    ref64 = float((((to64(y.cpu().numpy()) - to64(t.cpu().numpy())) * 255.0) ** 2).mean())
    assert abs(float(loss) - ref64) <= 1e-6 * ref64
    with pytest.raises(ValueError):
        ops.mse255_sum_s2d3(parts + parts + parts + parts + parts + parts + parts, y, t, 0.1)


@pytest.mark.parametrize('shape', [(3, 40, 56, 3), (2, 64, 64, 1), (1, 11, 11, 3)])
def test_ssim_both_flavours(dev, shape):
    """Device SSIM against the restated skimage (7x7 uniform, sample covariance) and tf.image.ssim (11x11 Gaussian)."""
    from neural_imaging_amd import ops
    from neural_imaging_amd.helpers import metrics
    n, h, w, c = shape
    a = natural_images(n, h, w, seed=5)[..., :c].copy()
    b = np.clip(a + rnd(a.shape, 6, -0.08, 0.08), 0, 1).astype(np.float32)
    got = ops.ssim(g(a, dev), g(b, dev), mode='skimage').cpu().numpy()
    ref = np.array([T.ssim_skimage(a[i], b[i]) for i in range(n)])
    assert np.abs(got - ref).max() < 1e-5, (got, ref)
    got_tf = ops.ssim(g(a, dev), g(b, dev), mode='tf').cpu().numpy()
    ref_tf = T.ssim_tf(to64(a), to64(b)).numpy()
    assert np.abs(got_tf - ref_tf).max() < 1e-5, (got_tf, ref_tf)
    assert np.abs(ops.ssim(g(a, dev), g(a, dev)).cpu().numpy() - 1.0).max() < 1e-6
    # reference surface (helpers/metrics.py): (H,W,C) -> scalar, (N,H,W,C) -> per image, batch() -> mean
    assert isinstance(metrics.ssim(a[0], b[0]), float) and abs(metrics.ssim(a[0], b[0]) - ref[0]) < 1e-5
    assert isinstance(metrics.ssim(a, b), float) if n == 1 else metrics.ssim(a, b).shape == (n,)
    assert abs(metrics.psnr(a[0], b[0]) - 10 * np.log10(1.0 / np.mean((a[0].astype(np.float64) - b[0]) ** 2))) < 1e-4
    if n > 1:
        assert abs(metrics.batch(a, b, metrics.ssim) - ref.mean()) < 1e-5


def test_edge_cases_empty_ragged_and_error_codes(dev):
    """Empty batches are no-ops, ragged (non-tile-multiple) sizes are exact, malformed calls come back as negative
    NIMG_ERR_* codes (surfaced as RuntimeError by the binding) instead of launching."""
    from neural_imaging_amd import _lib, ops
    # empty batch through the main entry points
    x0 = torch.empty((0, 16, 16, 8), device=dev)
    w = g(rnd((3, 3, 8, 16), 1), dev)
    assert ops.conv2d(x0, w).shape == (0, 16, 16, 16)
    assert ops.maxpool2(x0).shape == (0, 8, 8, 8)
    y0, m0, _, _ = ops.djpeg_fwd(torch.empty((0, 16, 16, 3), device=dev), ops.qtables_device(50, dev))
    assert y0.shape == (0, 16, 16, 3)
    # ragged sizes: 1 x 1 pixels, prime sizes, single channel counts around the vector widths
    for (n, h, wd, cin, cout, ks) in [(1, 1, 1, 8, 8, 3), (2, 7, 13, 5, 9, 3), (1, 17, 3, 12, 20, 5), (3, 9, 9, 1, 1, 5)]:
        x, wt, b = rnd((n, h, wd, cin), 2), rnd((ks, ks, cin, cout), 3, -0.3, 0.3), rnd((cout,), 4)
        ref = T.conv2d(to64(x), to64(wt), to64(b)).numpy()
        out = ops.conv2d(g(x, dev), g(wt, dev), g(b, dev))
        assert_close(out.cpu().numpy(), ref, 1e-5, GRTOL, what='ragged conv {}'.format((n, h, wd, cin, cout, ks)))
    # error codes: odd size into the pool, dJPEG on a size that is not a multiple of 8, bad activation id
    xo = rnd((1, 5, 7, 4), 5)                                 # odd sizes pool VALID: last row / column dropped
    yo = ops.maxpool2(g(xo, dev))
    ref_o = T.max_pool2(to64(xo)).numpy()
    assert yo.shape == (1, 2, 3, 4) and np.array_equal(yo.cpu().numpy(), ref_o.astype(np.float32))
    xt = to64(xo).requires_grad_(True)
    dpo = rnd((1, 2, 3, 4), 6)
    (T.max_pool2(xt) * to64(dpo)).sum().backward()
    dzo = ops.maxpool2_bwd(g(dpo, dev), g(xo, dev), None, apply_mask=False)
    assert_close(dzo.cpu().numpy(), xt.grad.numpy(), 1e-6, what='odd-size pool backward')
    with pytest.raises(RuntimeError):
        ops.djpeg_fwd(g(rnd((1, 12, 16, 3), 6), dev), ops.qtables_device(50, dev))
    lib = _lib.load()
    xx = g(rnd((1, 8, 8, 8), 7), dev)
    out = torch.empty((1, 8, 8, 16), device=dev)
    rc = lib.nimg_conv2d_fwd(xx.data_ptr(), 8, None, 0, w.data_ptr(), None, out.data_ptr(), 16, None, 0, None, 1, 8, 8, 3, 1, 1,
                             1, 0, 8, 8, 7, 0.2, None)
    assert rc < 0
    assert lib.nimg_conv2d_fwd(None, 8, None, 0, w.data_ptr(), None, out.data_ptr(), 16, None, 0, None, 1, 8, 8, 3, 1, 1, 1, 0,
                               8, 8, 0, 0.2, None) < 0
    # host tensors and non-contiguous tensors are refused - there is no CPU path
    with pytest.raises(RuntimeError):
        ops.conv2d(torch.zeros((1, 8, 8, 8)), w)
    with pytest.raises(RuntimeError):
        ops.conv2d(xx.permute(0, 2, 1, 3), w)


def test_d2s_clip_and_small_ops(dev):
    from neural_imaging_amd import ops
    x = rnd((2, 6, 5, 12), 1, -0.5, 1.5)
    ref = torch.clamp(T.depth_to_space(to64(x), 2), 0, 1)
    y = ops.d2s_clip(g(x, dev))
    assert np.array_equal(y.cpu().numpy(), ref.numpy().astype(np.float32))
    dy = rnd(tuple(ref.shape), 2)
    dx = ops.d2s_clip_bwd(g(dy, dev))
    assert np.array_equal(dx.cpu().numpy(), T.space_to_depth(to64(dy), 2).numpy().astype(np.float32))
    a, b = rnd((1000,), 3), rnd((1000,), 4)
    assert np.allclose(ops.add(g(a, dev), g(b, dev)).cpu().numpy(), a + b)
    assert np.allclose(ops.lrelu_bwd(g(a, dev), g(b, dev)).cpu().numpy(), a * np.where(b > 0, 1.0, 0.2))
    xx = rnd((2, 8, 8, 3), 5)
    assert_close(ops.avgpool(g(xx, dev), 2).cpu().numpy(), T.avg_pool(to64(xx), 2).numpy(), 1e-6, what='avgpool')
    dyy = rnd((2, 4, 4, 3), 6)
    assert_close(ops.avgpool_bwd(g(dyy, dev), 2).cpu().numpy(), np.repeat(np.repeat(dyy, 2, 1), 2, 2) / 4, 1e-6,
                 what='avgpool bwd')


def test_mse255_and_adam_and_nanflag(dev):
    from neural_imaging_amd import ops
    a, b = rnd((3, 16, 16, 3), 1, 0, 1), rnd((3, 16, 16, 3), 2, 0, 1)
    at = to64(a).requires_grad_(True)
    loss = T.mse255(at, to64(b))
    (0.1 * loss).backward()
    lo, gr = ops.mse255(g(a, dev), g(b, dev), grad_scale=0.1)
    assert abs(float(lo.item()) - float(loss)) / float(loss) < 1e-5
    assert_close(gr.cpu().numpy(), at.grad.numpy(), 1e-6, GRTOL, what='mse255 grad')
    # Keras Adam, 3 steps
    p0, grads = rnd((1000,), 3), [rnd((1000,), 10 + k) for k in range(3)]
    p = [to64(p0).clone()]
    m, v = [torch.zeros(1000, dtype=torch.float64)], [torch.zeros(1000, dtype=torch.float64)]
    pg, mg, vg = g(p0, dev), torch.zeros(1000, device=dev), torch.zeros(1000, device=dev)
    for k in range(3):
        T.adam_step(p, [to64(grads[k])], m, v, k + 1, 1e-3)
        ops.adam_step(pg, g(grads[k], dev), mg, vg, 1e-3, k + 1)
    assert_close(pg.cpu().numpy(), p[0].numpy(), 1e-6, what='adam params')
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.nan_flag(pg, flag)
    assert int(flag.item()) == 0
    pg[17] = float('nan')
    ops.nan_flag(pg, flag)
    assert int(flag.item()) == 1
    before = pg.clone()
    ops.adam_step(pg, g(grads[0], dev), mg, vg, 1e-3, 4, skip_flag=flag)      # skipped
    assert torch.equal(torch.nan_to_num(pg), torch.nan_to_num(before))


@pytest.mark.parametrize('k', [5, 16, 17, 100, 256])
def test_fan_head(dev, k):
    """GAP -> Dense(k, softmax) -> Keras sparse CE on probabilities, forward and backward: k <= 16 in one lane's registers, from
    17 classes on the lanes of the image's wave own the classes (the reference allows n_classes up to 256, forensics.py:37)."""
    from neural_imaging_amd import ops
    n, h, w, c = 6, 4, 4, 32
    act = to64(rnd((n, h, w, c), 1)).requires_grad_(True)
    wt = to64(rnd((c, k), 2)).requires_grad_(True)
    b = to64(rnd((k,), 3)).requires_grad_(True)
    labels = (np.array([0, 1, 2, 3, 4, 1], np.int32) * 53 + (k - 1) * np.array([0, 0, 1, 0, 0, 1], np.int32)) % k
    a = T.leaky_relu(act)
    probs = torch.softmax(a.mean(dim=(1, 2)) @ wt + b, dim=1)
    loss = T.sparse_ce_from_probs(probs, labels)
    loss.backward()
    a_np = a.detach().numpy()
    gap, pr, lp, dl = ops.fan_head_fwd(g(a_np, dev), g(wt.detach().numpy(), dev), g(b.detach().numpy(), dev),
                                       torch.from_numpy(labels).to(dev), 1.0 / n)
    assert_close(pr.cpu().numpy(), probs.detach().numpy(), 1e-6, what='probs')
    dw, db = torch.empty((c, k), device=dev), torch.empty((k,), device=dev)
    dact, lo = ops.fan_head_bwd(g(a_np, dev), gap, g(wt.detach().numpy(), dev), dl, lp, 1.0 / n, dw, db)
    assert abs(float(lo.item()) - float(loss)) < 1e-5
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 1e-6, GRTOL, what='dense dW')
    assert_close(db.cpu().numpy(), b.grad.numpy(), 1e-6, GRTOL, what='dense db')
    assert_close(dact.cpu().numpy(), act.grad.numpy(), 1e-7, GRTOL, what='d pre-activation of conv1x1')


# ------------------------------------------------------------------------------------------------------------------
# constrained conv + manipulations
def test_constrained_conv(dev):
    from neural_imaging_amd import ops
    k = to64(ot.fan_residual_init() + 0.05 * rnd((5, 5, 3, 3), 1)).requires_grad_(True)
    m = to64(ot.center_mask_2dfilter(5, 3))
    x = to64(natural_images(2, 24, 32, seed=4)).requires_grad_(True)
    y = T.constrained_conv(x, k, m)
    dy = rnd(tuple(y.shape), 2)
    (y * to64(dy)).sum().backward()
    kg = g(k.detach().numpy(), dev)
    nf = ops.constrained_kernel(kg)
    assert_close(nf.cpu().numpy(), T.constrained_kernel(k.detach(), m).numpy(), 1e-4, 1e-6, what='normalised filter')
    yo = ops.conv2d(g(x.detach().numpy(), dev), nf, None, pads=(2, 2), out_hw=(24, 32), pad_mode=1)
    assert_close(yo.cpu().numpy(), y.detach().numpy(), 1e-3, 1e-5, what='constrained conv fwd')
    dnf = ops.conv2d_wgrad(g(x.detach().numpy(), dev), g(dy, dev), 5, pads=(2, 2), pad_mode=1)
    dk = torch.empty_like(kg)
    ops.constrained_kernel_bwd(kg, dnf, dk)
    assert_close(dk.cpu().numpy(), k.grad.numpy(), 1e-4, GRTOL, what='constrained kernel grad')
    dpad = ops.conv2d(g(dy, dev), ops.flip_weights(nf), None, pads=(4, 4), out_hw=(28, 36))
    dx = ops.fold_pad(dpad, 2, 1)
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 1e-3, GRTOL, what='constrained conv input grad')


@pytest.mark.parametrize('shape', [(2, 24, 32), (1, 40, 272), (3, 8, 8), (1, 5, 100), (2, 256, 256)])
def test_cconv3_front_end_stencil(dev, shape):
    """csrc/frontend.hip: the ConstrainedConv2D forward (SYMMETRIC pad) and its input gradient (flipped filter + border
    fold) against the float64 oracle (models/layers.py:56-57), on both tile shapes (narrow / full-width), ragged sizes and the
    bench size; the bf16 {y, 1} pixel is the rounded float32 output."""
    from neural_imaging_amd import ops
    n, h, w = shape
    k = to64(ot.fan_residual_init() + 0.05 * rnd((5, 5, 3, 3), 1))
    m = to64(ot.center_mask_2dfilter(5, 3))
    x = to64(natural_images(n, h, w, seed=4)).requires_grad_(True)
    y = T.constrained_conv(x, k, m)
    dy = rnd(tuple(y.shape), 2)
    (y * to64(dy)).sum().backward()
    nf = ops.constrained_kernel(g(k.numpy(), dev))
    yo, c4 = ops.cconv3(g(x.detach().numpy(), dev), nf, pad_mode=1, want_c4=True)
    assert_close(yo.cpu().numpy(), y.detach().numpy(), 1e-3, 1e-5, what='constrained conv fwd')
    c4 = c4.float().cpu().numpy()
    assert np.array_equal(c4[..., :3], yo.to(torch.bfloat16).float().cpu().numpy()) and (c4[..., 3] == 1.0).all()
    dx = ops.cconv3_dgrad(g(dy, dev), nf)
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 1e-3, GRTOL, what='constrained conv input grad')
    # the previous decomposition (full correlation on the padded domain, then the fold) gives the same numbers
    dpad = ops.conv2d(g(dy, dev), ops.flip_weights(nf), None, pads=(4, 4), out_hw=(h + 4, w + 4), _f32_only=True)
    assert_close(dx.cpu().numpy(), ops.fold_pad(dpad, 2, 1).cpu().numpy(), 1e-3, 1e-5, what='vs pad-fold path')


@pytest.mark.parametrize('shape', [(2, 64, 64), (1, 40, 128), (3, 13, 192), (2, 256, 256), (1, 6, 64)])
def test_constrained_filter_wgrad_on_the_matrix_core(dev, shape):
    """csrc/conv_small.hip conv_wgrad_c3k5_mfma_kernel (throughput mode): the 5x5x3x3 weight gradient of the ConstrainedConv2D
    (SYMMETRIC pad, models/layers.py:56) as one 16 x 16 MFMA tile over bf16 operands - against the float64 oracle on the
    bf16-rounded operands (only the float32 accumulation order differs) and against the exact float32 kernel of the parity mode."""
    from neural_imaging_amd import ops
    n, h, w = shape
    x_np, dy_np = natural_images(n, h, w, seed=6), rnd((n, h, w, 3), 7)
    xr, dr = _bf16_round(x_np), _bf16_round(dy_np)
    k = to64(rnd((5, 5, 3, 3), 1)).requires_grad_(True)
    y = T.conv2d(T.pad2d(xr, 2, 'SYMMETRIC'), k, None, 1, 'VALID')
    (y * dr).sum().backward()
    ref = k.grad.numpy()
    ops.set_compute('bf16')
    try:
        dw = ops.conv2d_wgrad(g(x_np, dev), g(dy_np, dev), 5, pads=(2, 2), pad_mode=1)
        assert_close(dw.cpu().numpy(), ref, 1e-6, 2e-5, what='c3k5 wgrad, matrix core')
        dw2 = torch.full_like(dw, 1.0)
        ops.conv2d_wgrad(g(x_np, dev), g(dy_np, dev), 5, pads=(2, 2), pad_mode=1, dw=dw2, accumulate=True)
        assert_close((dw2 - 1.0).cpu().numpy(), ref, 1e-5, 2e-5, what='accumulate')
    finally:
        ops.set_compute('f32')
    exact = ops.conv2d_wgrad(g(x_np, dev), g(dy_np, dev), 5, pads=(2, 2), pad_mode=1)          # float32 operands, VALU
    scale = np.abs(exact.cpu().numpy()).max()
    assert np.abs(dw.cpu().numpy() - exact.cpu().numpy()).max() <= 1.5e-2 * scale


@pytest.mark.parametrize('shape', [(2, 24, 64), (1, 37, 128), (2, 256, 256), (1, 5, 192)])
def test_cconv3_input_gradient_on_the_matrix_core(dev, shape):
    """csrc/frontend.hip conv5c3_mfma_kernel (throughput mode): the main term of the ConstrainedConv2D input gradient as a banded
    bf16 matrix product - against the float64 oracle of the whole gradient (SYMMETRIC-pad fold included) evaluated on the
    bf16-rounded operands, and against the float32 stencil of the parity mode."""
    from neural_imaging_amd import ops
    n, h, w = shape
    k = to64(ot.fan_residual_init() + 0.05 * rnd((5, 5, 3, 3), 1))
    m = to64(ot.center_mask_2dfilter(5, 3))
    nf64 = T.constrained_kernel(k, m)
    nf = g(nf64.numpy(), dev)
    dy_np = rnd((n, h, w, 3), 2)
    x = to64(natural_images(n, h, w, seed=4)).requires_grad_(True)
    y = T.conv2d(T.pad2d(x, 2, 'SYMMETRIC'), _bf16_round(nf64.numpy()), None, 1, 'VALID')
    (y * _bf16_round(dy_np)).sum().backward()
    exact = ops.cconv3_dgrad(g(dy_np, dev), nf)                    # float32 stencil
    ops.set_compute('bf16')
    try:
        dx = ops.cconv3_dgrad(g(dy_np, dev), nf)
    finally:
        ops.set_compute('f32')
    # interior: bf16 operands on both sides; the 2-pixel border adds the float32 mirror terms (nimg_cconv3_dgrad_border)
    ref = x.grad.numpy()
    assert_close(dx.cpu().numpy()[:, 2:-2, 2:-2], ref[:, 2:-2, 2:-2], 1e-4, 1e-5, what='matrix-core dgrad, interior')
    scale = np.abs(exact.cpu().numpy()).max()
    assert np.abs(dx.cpu().numpy() - exact.cpu().numpy()).max() <= 1.5e-2 * scale


def _bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).double()


def unpack_argmax2(p):
    """(..., 8) uint8 codes of nimg_conv1_pool_fwd_c4 -> (..., 32) arg-max positions: channel c = byte c >> 2, bits 2 (c & 3)."""
    c = np.arange(32)
    return (p[..., c >> 2] >> (2 * (c & 3))) & 3


def pack_argmax2(k):
    p = np.zeros(k.shape[:-1] + (8,), np.uint8)
    for c in range(32):
        p[..., c >> 2] |= (k[..., c].astype(np.uint8) & 3) << (2 * (c & 3))
    return p


@pytest.mark.parametrize('shape,out_bf16', [((2, 16, 32), False), ((1, 24, 72), True), ((3, 64, 64), True), ((1, 10, 256), False),
                                            ((2, 256, 256), True)])
def test_conv1_pool_front_end(dev, shape, out_bf16):
    """csrc/frontend.hip conv1_pool_fwd_kernel: Conv2D(32, 5x5, SAME) + bias + LeakyReLU + MaxPool2D over 8-byte bf16 pixels
    (models/forensics.py:69-70) against the float64 oracle evaluated on the SAME bf16-rounded operands (so only the float32
    accumulation order differs): pooled values, and the arg-max byte wherever the window maximum is not a near-tie."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    n, h, w = shape
    c = rnd((n, h, w, 3), 11) * 2.0
    wk = rnd((5, 5, 3, 32), 12) * 0.2
    b = rnd((32,), 13) * 0.1
    c4 = torch.ones((n, h, w, 4), dtype=torch.bfloat16, device=dev)
    c4[..., :3] = g(c, dev).to(torch.bfloat16)
    pooled, idx = ops.conv1_pool_c4(c4.contiguous(), g(wk, dev), g(b, dev), out_bf16=out_bf16)
    act = T.leaky_relu(T.conv2d(_bf16_round(c), _bf16_round(wk), to64(b)))
    ref = T.max_pool2(act).numpy()
    got = pooled.float().cpu().numpy()
    tol = 1e-2 if out_bf16 else 2e-4                         # bf16 storage rounds to 2^-9 relative
    assert got.shape == ref.shape == (n, h // 2, w // 2, 32)
    assert np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()
    win = act.numpy().reshape(n, h // 2, 2, w // 2, 2, 32).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, 32, 4)
    srt = np.sort(win, axis=-1)
    clear = (srt[..., 3] - srt[..., 2]) > 1e-4 * (1.0 + np.abs(srt[..., 3]))
    assert tuple(idx.shape) == (n, h // 2, w // 2, 8)
    k = unpack_argmax2(idx.cpu().numpy())
    assert clear.mean() > 0.99 and np.array_equal(k[clear], win.argmax(axis=-1)[clear]) and k.max() <= 3
    # same kernel, no activation (alpha = 1) and no bias / no arg-max output
    p2, i2 = ops.conv1_pool_c4(c4.contiguous(), g(wk, dev), None, act=None, want_idx=False, out_bf16=out_bf16)
    ref2 = T.max_pool2(T.conv2d(_bf16_round(c), _bf16_round(wk), None)).numpy()
    assert i2 is None and np.abs(p2.float().cpu().numpy() - ref2).max() <= tol * max(1.0, np.abs(ref2).max())


@pytest.mark.parametrize('shape,g_bf16', [((2, 16, 32), False), ((1, 24, 72), True), ((3, 64, 64), True), ((1, 10, 256), False),
                                          ((2, 256, 256), True)])
def test_conv1_wgrad_front_end(dev, shape, g_bf16):
    """csrc/frontend.hip conv1_wgrad_pooled_kernel: weight + bias gradient of the FAN's first convolution from the pooled
    gradient and the arg-max bytes, against float64 autograd on the same bf16-rounded operands (MaxPool2D routing restated)."""
    from neural_imaging_amd import ops
    n, h, w = shape
    c = _bf16_round(rnd((n, h, w, 3), 21) * 2.0)
    gp = _bf16_round(rnd((n, h // 2, w // 2, 32), 22))
    k = np.random.default_rng(23).integers(0, 4, size=(n, h // 2, w // 2, 32)).astype(np.uint8)
    dz = np.zeros((n, h, w, 32))
    for pos in range(4):
        dz[:, pos >> 1::2, pos & 1::2, :] = np.where(k == pos, gp.numpy(), 0.0)
    wk = to64(rnd((5, 5, 3, 32), 24)).requires_grad_(True)
    (T.conv2d(c, wk, None) * to64(dz)).sum().backward()
    c4 = torch.ones((n, h, w, 4), dtype=torch.bfloat16, device=dev)
    c4[..., :3] = c.to(torch.bfloat16).to(dev)
    gd = gp.to(torch.bfloat16 if g_bf16 else torch.float32).to(dev).contiguous()
    dw = torch.full((5, 5, 3, 32), 7.0, device=dev)
    db = torch.full((32,), 7.0, device=dev)
    ops.conv1_wgrad_c4(c4.contiguous(), gd, torch.from_numpy(pack_argmax2(k)).to(dev), dw=dw, db=db)
    assert_close(dw.cpu().numpy(), wk.grad.numpy(), 1e-6, 2e-5, what='conv1 dw')
    assert_close(db.cpu().numpy(), dz.sum(axis=(0, 1, 2)), 1e-6, 2e-5, what='conv1 db')
    ops.conv1_wgrad_c4(c4.contiguous(), gd, torch.from_numpy(pack_argmax2(k)).to(dev), dw=dw, db=db, accumulate=True)
    assert_close(dw.cpu().numpy(), 2 * wk.grad.numpy(), 1e-6, 4e-5, what='conv1 dw, accumulated')
    # input gradient from the same pooled gradient (conv1_dgrad_pooled_kernel): autograd w.r.t. the image, bf16-rounded kernel
    cx = c.clone().requires_grad_(True)
    wb = _bf16_round(wk.detach().numpy())
    (T.conv2d(cx, wb, None) * to64(dz)).sum().backward()
    dc = ops.conv1_dgrad_pooled(gd, torch.from_numpy(pack_argmax2(k)).to(dev), g(wk.detach().numpy(), dev))
    assert_close(dc.cpu().numpy(), cx.grad.numpy(), 1e-6, 2e-5, what='conv1 input gradient')


@pytest.mark.parametrize('name', ['gaussian', 'gaussian3', 'sharpen', 'sharpen_strong', 'resample50', 'resample73'])
def test_manipulations_fwd_bwd(dev, name):
    from neural_imaging_amd.helpers import tf_helpers as th
    x_np = natural_images(2, 32, 32, seed=7)
    if name.startswith('sharpen'):
        x_np = np.clip(x_np * 1.3 - 0.1, 0, 1).astype(np.float32)       # exercise the hard clip too
    x = to64(x_np).requires_grad_(True)
    if name == 'gaussian':
        op, s, ref = th.Gaussian(), 0.83, om.manipulation_gaussian(x, 5, 0.83)
    elif name == 'gaussian3':
        op, s, ref = th.Gaussian(), 3.0, om.manipulation_gaussian(x, 5, 3.0)
    elif name == 'sharpen':
        op, s, ref = th.Sharpen(), 1.0, om.manipulation_sharpen(x, 1.0)
    elif name == 'sharpen_strong':
        op, s, ref = th.Sharpen(), 1.5, om.manipulation_sharpen(x, 1.5)
    elif name == 'resample50':
        op, s, ref = th.Resample(), 50, om.manipulation_resample(x, 50)
    else:
        op, s, ref = th.Resample(), 73, om.manipulation_resample(x, 73)
    dy = rnd(tuple(ref.shape), 3)
    (ref * to64(dy)).sum().backward()
    y, ctx = op.forward(g(x_np, dev), s, training=True)
    assert_close(y.cpu().numpy(), ref.detach().numpy(), ATOL, what=name + ' fwd')
    dx = op.backward(ctx, g(dy, dev))
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 2e-4, 3e-4, what=name + ' bwd')


@pytest.mark.parametrize('name', ['gaussian3x3', 'gaussian7x7', 'gaussian9x9_noclip', 'gaussian1x1', 'sharpen_rgb',
                                  'sharpen_rgb_strong', 'residual', 'nearest50', 'nearest30'])
def test_manipulations_general_forms(dev, name):
    """The forms of the manipulations the workflow does not use (tf_helpers.py:68-184 with kernel != 5, hsv=False,
    method='nearest'), through both the objects (forward + backward) and the reference-named functions."""
    from neural_imaging_amd.helpers import tf_helpers as th
    hw = (20, 20) if name.startswith('nearest') else (24, 18)
    x_np = np.ascontiguousarray(natural_images(2, 24, 24, seed=11)[:, :hw[0], :hw[1]])
    if name.startswith('sharpen'):
        x_np = np.clip(x_np * 1.3 - 0.1, 0, 1).astype(np.float32)       # exercise the hard clip too
    x = to64(x_np).requires_grad_(True)
    xd = g(x_np, dev)
    if name.startswith('gaussian'):
        k = int(name[8])
        noclip = name.endswith('noclip')
        std = 1.7 if k > 3 else 0.6
        ref = om.manipulation_gaussian(x, k, std, skip_clip=noclip)
        op = th.Gaussian(k)
        y, ctx = op.forward(xd, std, training=True, skip_clip=noclip)
        fn = th.manipulation_gaussian(xd, k, std, skip_clip=noclip)
    elif name.startswith('sharpen'):
        s = 2.5 if name.endswith('strong') else 1.0
        ref = om.manipulation_sharpen(x, s, hsv=False)
        op = th.Sharpen(hsv=False)
        y, ctx = op.forward(xd, s, training=True)
        fn = th.manipulation_sharpen(xd, s, hsv=False)
    elif name == 'residual':
        ref = om.residual(x)
        op = th.Residual()
        y, ctx = op.forward(xd, training=True)
        fn = th.residual(xd)
    else:
        f = int(name[7:])
        ref = om.manipulation_resample(x, f, 'nearest')
        op = th.Resample('nearest')
        y, ctx = op.forward(xd, f, training=True)
        fn = th.manipulation_resample(xd, f, 'nearest')
    dy = rnd(tuple(ref.shape), 3)
    (ref * to64(dy)).sum().backward()
    assert_close(y.cpu().numpy(), ref.detach().numpy(), ATOL, what=name + ' fwd')
    assert np.array_equal(fn.t.cpu().numpy(), y.cpu().numpy()), 'function and object forms differ'
    dx = op.backward(ctx, g(dy, dev))
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 2e-4, 3e-4, what=name + ' bwd')


@pytest.mark.parametrize('factor', [50, 73, 130])
@pytest.mark.parametrize('method', ['bicubic', 'area', 'lanczos3', 'lanczos5', 'gaussian', 'mitchellcubic'])
def test_resample_with_every_resize_method(dev, method, factor):
    """manipulation_resample(x, factor, method) for the method strings tf.image.resize takes besides bilinear / nearest
    (helpers/tf_helpers.py:68-76 passes `method` through; VERDICT r04 missing 4): down and back up, forward and input gradient,
    object and function forms, against the oracle's restatement of TensorFlow's kernels (oracle/tfops.py RESIZE_AXIS - built
    independently of the product's helpers/kernels.py; TensorFlow itself is not in the image: parity unpinned, like every TF op)."""
    from neural_imaging_amd.helpers import tf_helpers as th
    x_np = natural_images(2, 40, 40, seed=13)
    x = to64(x_np).requires_grad_(True)
    xd = g(x_np, dev)
    ref = om.manipulation_resample(x, factor, method)
    op = th.Resample(method)
    y, ctx = op.forward(xd, factor, training=True)
    fn = th.manipulation_resample(xd, factor, method)
    dy = rnd(tuple(ref.shape), 3)
    (ref * to64(dy)).sum().backward()
    assert_close(y.cpu().numpy(), ref.detach().numpy(), ATOL, what='{} {} fwd'.format(method, factor))
    assert np.array_equal(fn.t.cpu().numpy(), y.cpu().numpy()), 'function and object forms differ'
    dx = op.backward(ctx, g(dy, dev))
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 2e-4, 3e-4, what='{} {} bwd'.format(method, factor))


def test_manipulations_unbuilt_forms_raise(dev):
    from neural_imaging_amd.helpers import tf_helpers as th
    x = g(natural_images(1, 16, 16, seed=2), dev)
    with pytest.raises(NotImplementedError):
        th.manipulation_resample(x, 50, 'trilinear')                         # not a tf.image.ResizeMethod either
    with pytest.raises(ValueError):
        th.manipulation_gaussian(x, 4, 1.0)
    with pytest.raises(RuntimeError):
        th.manipulation_gaussian(x[:, :3, :3].contiguous(), 9, 1.0)           # nothing to mirror: refused by the C ABI


@pytest.mark.parametrize('hw', [(24, 40), (16, 16), (50, 18), (8, 12), (16, 64), (32, 128), (48, 192)])
def test_gaussian_backward_tiled_and_plain(dev, hw):
    """The LDS-tiled kernels (images >= 16x16, partial border tiles), their wide form (h % 16 == 0, w % 64 == 0: one, two and
    three tiles per row, mirrored borders inside and across tiles) and the plain kernels (smaller images) against autograd
    through the REFLECT-padded filter."""
    from neural_imaging_amd.helpers import tf_helpers as th
    h, w = hw
    x_np = np.ascontiguousarray(natural_images(2, max(h, w), max(h, w), seed=9)[:, :h, :w])    # no saturated regions:
    # a float32 blur of an all-ones window can land 1 ulp above 1 and flip the clip mask against the float64 oracle
    x = to64(x_np).requires_grad_(True)
    ref = om.manipulation_gaussian(x, 5, 0.83)
    dy = rnd(tuple(ref.shape), 3)
    (ref * to64(dy)).sum().backward()
    op = th.Gaussian()
    y, ctx = op.forward(g(x_np, dev), 0.83, training=True)
    assert_close(y.cpu().numpy(), ref.detach().numpy(), ATOL, what='gaussian fwd')
    dx = op.backward(ctx, g(dy, dev))
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 2e-4, 3e-4, what='gaussian bwd {}'.format(hw))


# ------------------------------------------------------------------------------------------------------------------
# learned-codec pieces
def test_latent_soft_codebook_and_entropy(dev):
    """DiscreteLatent (models/layers.py:183-203): latent values, batch-global entropy and their gradients."""
    from neural_imaging_amd import ops
    cb = ot.codebook(5)
    z_np = (rnd((2, 4, 4, 32), 1) * 6).astype(np.float32)
    z = to64(z_np).requires_grad_(True)
    s = torch.tensor(1.3, dtype=torch.float64, requires_grad=True)
    lat = T.soft_codebook(z.to(torch.float32).to(torch.float64) * s, to64(cb))
    ent, _ = T.entropy(lat, to64(cb))
    dl = rnd(z_np.shape, 2)
    loss = (lat * to64(dl)).sum() + 250.0 * ent
    loss.backward()
    ws = ops.LatentWorkspace(32, dev)
    sc = torch.tensor([1.3], dtype=torch.float32, device=dev)
    lg, eg = ops.latent_fwd(g(z_np, dev), sc, g(cb, dev), ws)
    assert np.array_equal(np.round(lg.cpu().numpy()), np.round(lat.detach().numpy())), 'hard codebook indices differ'
    assert_close(lg.cpu().numpy(), lat.detach().numpy(), 1e-5, what='latent')
    assert abs(float(eg.item()) - float(ent)) < 1e-5
    dscale = torch.zeros(1, device=dev)
    dz = ops.latent_bwd(g(z_np, dev), sc, lg, g(dl, dev), 250.0, g(cb, dev), ws, dscale=dscale)
    assert_close(dz.cpu().numpy(), z.grad.numpy(), 1e-6, 2e-4, what='latent dz')
    assert abs(float(dscale.item()) - float(s.grad)) / (abs(float(s.grad)) + 1e-9) < 2e-4
    # entropy KATs on the device: constant latent -> ~0 bits, uniform over the 32 centres -> ~5 bits
    one = torch.ones(1, device=dev)
    _, e0 = ops.latent_fwd(torch.zeros(4096, device=dev), one, g(cb, dev), ws)
    _, e5 = ops.latent_fwd(g(np.tile(cb, 128), dev), one, g(cb, dev), ws)
    assert float(e0.item()) < 1e-4 and abs(float(e5.item()) - 5.0) < 1e-3
    # the windowed kernels (unit_codebook promise: only the five centres around the nearest one are evaluated inside the codebook's
    # range) against the full ones AND the oracle: values at centres, at midpoints between centres, at the range ends and far
    # outside (there the full loop runs)
    zw = np.concatenate([cb, cb[:-1] + 0.5, cb[:-1] + 0.4999, [cb[0] - 0.5, cb[0] - 0.51, cb[-1] + 0.5, cb[-1] + 0.6,
                                                                 -40.0, 55.0, cb[0] - 3.0], (rnd((400,), 5) * 20)]).astype(np.float32)
    dlw = rnd(zw.shape, 6)
    zt = to64(zw).requires_grad_(True)
    latw = T.soft_codebook(zt, to64(cb))
    entw, _ = T.entropy(latw, to64(cb))
    ((latw * to64(dlw)).sum() + 250.0 * entw).backward()
    res = {}
    for unit in (False, True):
        l_, e_ = ops.latent_fwd(g(zw, dev), one, g(cb, dev), ws, unit_codebook=unit)
        d_ = ops.latent_bwd(g(zw, dev), one, l_, g(dlw, dev), 250.0, g(cb, dev), ws, dscale=dscale, unit_codebook=unit)
        res[unit] = (l_.cpu().numpy(), float(e_.item()), d_.cpu().numpy(), float(dscale.item()))
    assert np.array_equal(res[True][0], res[False][0]) and abs(res[True][1] - res[False][1]) < 1e-7
    assert_close(res[True][2], res[False][2], 1e-9, 1e-6, what='windowed vs full dz')
    assert abs(res[True][3] - res[False][3]) <= 1e-6 * abs(res[False][3]) + 1e-9
    assert_close(res[True][0], latw.detach().numpy(), 1e-5, what='windowed latent vs oracle')
    assert abs(res[True][1] - float(entw)) < 1e-5
    assert_close(res[True][2], zt.grad.numpy(), 1e-6, 2e-4, what='windowed dz vs oracle')


@pytest.mark.parametrize('shape', [(2, 32, 48, 3, 64), (1, 16, 16, 8, 16), (2, 24, 40, 64, 32)])
def test_stride2_conv_as_space_to_depth_conv(dev, shape):
    """A 5x5 stride-2 TF-SAME layer evaluated as a 3x3 stride-1 layer over the space-to-depth image (csrc/latent.hip s2d kernels,
    models/layers.py Conv5x5Stride2Image; models/compression.py:217-229): forward, weight / bias gradient and input gradient
    against float64 autograd through the strided convolution on the same bf16-rounded operands."""
    from neural_imaging_amd import ops
    from neural_imaging_amd.models.layers import Conv5x5Stride2Image
    from neural_imaging_amd.models.tfmodel import ParamStore
    ops.set_compute('bf16')
    try:
        n, h, w, cin, cout = shape
        img = rnd((n, h, w, cin), 31, 0.0, 1.0)
        wk = rnd((5, 5, cin, cout), 32, -0.2, 0.2)
        b = rnd((cout,), 33, -0.1, 0.1)
        x0 = _bf16_round(2.0 * img.astype(np.float32) - 1.0).requires_grad_(True)        # what the bf16 block image holds
        wr = _bf16_round(wk).requires_grad_(True)
        bb = to64(b).requires_grad_(True)
        ref = T.conv2d(x0, wr, bb, 2, 'SAME')
        dz = rnd(tuple(ref.shape), 34)
        (ref * to64(dz)).sum().backward()
        # the weight transform and its adjoint
        w3 = ops.s2d_conv_weights(g(wk, dev))
        cp = w3.shape[2]
        assert cp % 16 == 0 and cp >= 4 * cin and float(w3.abs().sum()) == pytest.approx(float(np.abs(wk).sum()), rel=1e-5)
        assert np.array_equal(w3.cpu().numpy(), T.s2d_conv_weights(torch.from_numpy(wk), cp).numpy())      # the oracle's statement of it
        probe = rnd((3, 3, cp, cout), 35)
        back = ops.s2d_conv_weights_bwd(g(probe, dev), torch.zeros((5, 5, cin, cout), device=dev))
        assert abs(float((w3 * g(probe, dev)).sum()) - float((back * g(wk, dev)).sum())) < 1e-3          # <T w, p> == <w, T^t p>
        if cin == 3:
            layer = Conv5x5Stride2Image('e1', 5, 3, cout, None, stride=2)
            store = ParamStore(layer.specs(), dev)
            store.p['e1/kernel'].copy_(g(wk, dev))
            store.p['e1/bias'].copy_(g(b, dev))
            y, ctx = layer.forward_image(store, g(img, dev), 2.0, -1.0)
            assert ctx.dtype == torch.bfloat16 and tuple(ctx.shape) == (n, h // 2, w // 2, 16)
            assert_close(y.cpu().numpy(), ref.detach().numpy(), 2e-3, 1e-3, what='s2d forward')
            layer.backward_params_image(store, ctx, g(dz, dev))
            ops.join_side_stream()
            assert_close(store.g['e1/kernel'].cpu().numpy(), wr.grad.numpy(), 2e-3, 1e-2, what='s2d weight gradient')
            assert_close(store.g['e1/bias'].cpu().numpy(), bb.grad.numpy(), 1e-4, 1e-3, what='s2d bias gradient')
            dx = layer.backward_input_image(store, g(dz, dev), (h, w), 2.0)
            assert_close(dx.cpu().numpy(), 2.0 * x0.grad.numpy(), 2e-3, 1e-2, what='s2d input gradient of the image layer')
        else:
            dxs = ops.conv2d_dgrad_strided2(g(dz, dev), g(wk, dev), (h, w))
            assert_close(dxs.cpu().numpy(), x0.grad.numpy(), 2e-3, 1e-2, what='s2d input gradient')
    finally:
        ops.set_compute('f32')


def test_strided_layer_on_a_space_to_depth_stored_input(dev):
    """models/compression.py:217-220 in throughput mode: the first layer's activation exists only as its bf16 space-to-depth
    image; the 5x5 stride-2 layer behind it runs forward and weight gradient as a 3x3 layer on that image (Conv2D.forward_s2d /
    backward_params_s2d) and masks its input gradient with it (NIMG_MASK_CONV).  Against float64 autograd through the strided
    convolution of the bf16-rounded activation."""
    from neural_imaging_amd import ops
    from neural_imaging_amd.models.layers import Conv2D
    from neural_imaging_amd.models.tfmodel import ParamStore
    n, h, w, cin, cout = 2, 32, 48, 16, 32                     # h x w = the resolution of the activation e1
    ops.set_compute('bf16')
    try:
        layer = Conv2D('e2', 5, cin, cout, None, stride=2)
        assert layer.s2d_chain_ok((h, w)) and not layer.s2d_chain_ok((h + 1, w))
        store = ParamStore(layer.specs(), dev)
        wk, b = rnd((5, 5, cin, cout), 71, -0.1, 0.1), rnd((cout,), 72, -0.1, 0.1)
        store.p['e2/kernel'].copy_(g(wk, dev))
        store.p['e2/bias'].copy_(g(b, dev))
        e1 = rnd((n, h, w, cin), 73, -1.0, 1.0)
        e1r = _bf16_round(e1).requires_grad_(True)            # what the bf16 image holds
        wr = _bf16_round(wk).requires_grad_(True)
        bb = to64(b).requires_grad_(True)
        ref = T.conv2d(e1r, wr, bb, 2, 'SAME')
        dz = rnd(tuple(ref.shape), 74)
        dzr = _bf16_round(dz)
        (ref * dzr).sum().backward()
        e1s = g(T.space_to_depth(torch.from_numpy(e1), 2).numpy(), dev).to(torch.bfloat16)
        y, act = layer.forward_s2d(store, e1s, bf16_copy=True, copy_lrelu=True)
        assert_close(y.cpu().numpy(), ref.detach().numpy(), 2e-3, 1e-3, what='forward on the s2d image')
        assert torch.equal(act, ops.lrelu(y).to(torch.bfloat16))
        dzb = g(dz, dev).to(torch.bfloat16)
        layer.backward_params_s2d(store, e1s, dzb)
        ops.join_side_stream()
        assert_close(store.g['e2/kernel'].cpu().numpy(), wr.grad.numpy(), 2e-3, 1e-2, what='weight gradient on the s2d image')
        assert_close(store.g['e2/bias'].cpu().numpy(), dzr.sum((0, 1, 2)).numpy(), 1e-4, 1e-3, what='bias gradient')
        # input gradient x LeakyReLU'(e1), the mask read from the s2d image; stored as bf16 or float32
        want = e1r.grad * torch.where(e1r.detach() > 0, 1.0, 0.2)
        for out_bf16 in (False, True):
            d = layer.backward_input(store, dzb, (h, w), act_mask=e1s, out_bf16=out_bf16, mask_s2d=True)
            assert d.dtype == (torch.bfloat16 if out_bf16 else torch.float32) and tuple(d.shape) == (n, h, w, cin)
            assert_close(d.float().cpu().numpy(), want.numpy(), 1e-2 if out_bf16 else 2e-3, 1e-2, what='masked input gradient')
        plain = layer.backward_input(store, dzb, (h, w), act_mask=g(e1, dev))      # the float32, depth-to-space-layout mask
        assert torch.equal(plain, layer.backward_input(store, dzb, (h, w), act_mask=e1s, mask_s2d=True))
    finally:
        ops.set_compute('f32')


def test_conv3x3_writing_its_depth_to_space_image(dev):
    """NIMG_D2S_OUT: a 3x3 convolution whose epilogue stores tf.nn.depth_to_space(out, 2) (models/compression.py:233,245) - the
    forward layers d512 / d256 (bias + LeakyReLU before the permutation) and the input gradient of a stride-2 layer over its
    space-to-depth image (mask indexed in the output layout) - equals convolution -> d2s_clip (-> lrelu_bwd) bit for bit; the
    float32 mode runs exactly that sequence.  The 16-byte d2s / s2d kernels are checked against the per-element forms."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = 2, 12, 20, 32, 64
    x = g(rnd((n, h, w, cin), 51), dev)
    wk, b = g(rnd((3, 3, cin, cout), 52, -0.1, 0.1), dev), g(rnd((cout,), 53, -0.1, 0.1), dev)
    mask = g(rnd((n, 2 * h, 2 * w, cout // 4), 54), dev)
    d2s_ref = lambda t: T.depth_to_space(t.double().cpu(), 2).float()
    for mode in ('bf16', 'f32'):
        ops.set_compute(mode)
        try:
            for act in (None, 'leaky_relu'):
                plain = ops.conv2d(x, wk, b, act=act)
                fused = ops.conv2d(x, wk, b, act=act, d2s_out=True)
                assert tuple(fused.shape) == (n, 2 * h, 2 * w, cout // 4)
                assert torch.equal(fused.cpu(), d2s_ref(plain)), (mode, act)
            # input gradient of a stride-2 5x5 layer: (n, 2h, 2w, 16) <- dz (n, h, w, 32), masked by the layer's input
            w5 = g(rnd((5, 5, 16, 32), 55, -0.1, 0.1), dev)
            dz = g(rnd((n, h, w, 32), 56), dev)
            d_fused = ops.conv2d_dgrad_strided2(dz, w5, (2 * h, 2 * w), act_mask=mask)
            d_plain = ops.conv2d_dgrad_strided2(dz, w5, (2 * h, 2 * w))
            assert torch.equal(d_fused, ops.lrelu_bwd(d_plain, mask)), mode
            if mode == 'bf16':
                w3 = ops.s2d_conv_weights(w5)
                two_pass = ops.d2s2_scale(ops.conv2d_dgrad(dz, w3, (h, w)), 16, 1.0)
                assert torch.equal(d_plain, two_pass)
            # NIMG_S2D_OUT: an input gradient written as space_to_depth(gradient) - what the depth_to_space layer in front of
            # the convolution hands back to ITS producer - with mask and skip gradient in the convolution's own layout
            m64, r64 = g(rnd((n, h, w, 64), 62), dev), g(rnd((n, h, w, 64), 63), dev)
            s2d_ref = lambda t: T.space_to_depth(t.float().cpu(), 2)
            for cg in (12, 16):                                  # 12: the codec's last layer (64 -> 12 channels)
                gz = g(rnd((n, h, w, cg), 60 + cg), dev)
                wz = g(rnd((3, 3, 64, cg), 61 + cg, -0.1, 0.1), dev)
                for kw in (dict(act_mask=m64), dict(residual=r64), dict()):
                    ref = ops.conv2d_dgrad(gz, wz, (h, w), **kw)
                    got = ops.conv2d_dgrad(gz, wz, (h, w), s2d_out=True, **kw)
                    assert tuple(got.shape) == (n, h // 2, w // 2, 256)
                    assert torch.equal(got.cpu(), s2d_ref(ref)), (mode, cg, sorted(kw))
                    if mode == 'bf16' and (cg % 8 == 0 or 'residual' not in kw):      # the shapes the fused epilogue serves
                        gotb = ops.conv2d_dgrad(gz, wz, (h, w), s2d_out=True, out_bf16=True, **kw)
                        assert gotb.dtype == torch.bfloat16 and torch.equal(gotb.cpu(), s2d_ref(ref).to(torch.bfloat16))
        finally:
            ops.set_compute('f32')
    for c in (4, 64, 6):            # 16-byte kernels (c % 4 == 0) and the per-element form
        t = g(rnd((3, 6, 10, 4 * c), 57 + c, -0.5, 1.5), dev)
        for scale, shift, clip in ((1.0, 0.0, False), (0.5, 0.5, True)):
            y = ops.d2s_clip(t, scale, shift, clip)
            ref = scale * T.depth_to_space(t.cpu(), 2) + shift
            ref = ref.clamp(0.0, 1.0) if clip else ref
            assert torch.equal(y.cpu(), ref), (c, clip)
        dy = g(rnd((3, 12, 20, c), 58 + c), dev)
        back = ops.d2s_clip_bwd(dy, 0.5)
        assert tuple(back.shape) == (3, 6, 10, 4 * c)
        assert torch.equal(T.depth_to_space(back.cpu(), 2), 0.5 * dy.cpu()), c


def test_conv5x5_bf16_copy_at_ring_shapes(dev):
    """a 5x5 stride-1 layer over a bf16-stored input whose shape selects the ring kernels (Cout % 128 == 0, Cout % 64
    == 0 with H >= 32, Cout == 32) asked for the second bf16 copy of its float32 result.  The ring epilogue does not write that
    copy, so the dispatch must keep such a call on the generic kernel: the copy is the float32 result rounded to bf16, and the
    float32 result equals the plain call's (which does run the ring kernel) to summation order."""
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    try:
        for cin, cout, hw in ((32, 128, 32), (16, 64, 32), (32, 32, 32)):
            x = g(rnd((2, hw, hw, cin), 61 + cout), dev).to(torch.bfloat16)
            wk, b = g(rnd((5, 5, cin, cout), 62, -0.05, 0.05), dev), g(rnd((cout,), 63, -0.1, 0.1), dev)
            plain = ops.conv2d(x, wk, b, act='leaky_relu')
            both, copy = ops.conv2d(x, wk, b, act='leaky_relu', bf16_copy=True)
            assert copy is not None and copy.dtype == torch.bfloat16
            assert torch.equal(copy, both.to(torch.bfloat16)), (cin, cout)
            assert_close(both.cpu().numpy(), plain.cpu().numpy(), 1e-5, 1e-5, what='5x5 bf16_copy vs the ring kernel')
    finally:
        ops.set_compute('f32')


def test_conv3x3_with_fused_residual(dev):
    """nimg_conv2d_fwd_bf16_res: the skip connection of a residual block added in the convolution's epilogue - forward
    (net + conv(a) + bias) and input gradient (d_net + mask * dgrad) - equals the separate convolution followed by ops.add,
    bit for bit; parity mode falls back to exactly that pair."""
    from neural_imaging_amd import ops
    n, h, w, c = 2, 24, 40, 32
    x, r = g(rnd((n, h, w, c), 41), dev), g(rnd((n, h, w, c), 42), dev)
    wk, b = g(rnd((3, 3, c, c), 43, -0.1, 0.1), dev), g(rnd((c,), 44, -0.1, 0.1), dev)
    mask = g(rnd((n, h, w, c), 45), dev)
    for mode in ('bf16', 'f32'):
        ops.set_compute(mode)
        try:
            plain = ops.conv2d(x, wk, b)
            fused = ops.conv2d(x, wk, b, residual=r)
            assert torch.equal(fused, plain + r), mode
            dplain = ops.conv2d_dgrad(x, wk, (h, w), act_mask=mask)
            dfused = ops.conv2d_dgrad(x, wk, (h, w), act_mask=mask, residual=r)
            assert torch.equal(dfused, dplain + r), mode
            # the bf16 copy written next to the float32 result: that result rounded to nearest-even, nothing else - and a
            # convolution reading the copy equals the convolution reading the float32 tensor (which rounds on its way in)
            for res in (r, None):
                both, copy = ops.conv2d(x, wk, b, residual=res, bf16_copy=True)
                assert torch.equal(both, fused if res is not None else plain), mode
                dboth, dcopy = ops.conv2d_dgrad(x, wk, (h, w), act_mask=mask, residual=res, bf16_copy=True)
                assert torch.equal(dboth, dfused if res is not None else dplain), mode
                if mode == 'bf16':
                    assert copy.dtype == torch.bfloat16 and torch.equal(copy, both.to(torch.bfloat16))
                    assert torch.equal(dcopy, dboth.to(torch.bfloat16))
                    assert_close(ops.conv2d(copy, wk, b).cpu().numpy(), ops.conv2d(both, wk, b).cpu().numpy(), 1e-5, 1e-5,
                                 what='conv of the bf16 copy')        # same operands, the kernels' summation orders
                    dw_c = ops.conv2d_wgrad(copy, dcopy, 3)
                    dw_f = ops.conv2d_wgrad(both, dboth, 3)
                    assert_close(dw_c.cpu().numpy(), dw_f.cpu().numpy(), 1e-6, 2e-5, what='wgrad from the bf16 copies')
                else:
                    assert copy is None and dcopy is None           # float32 mode has no bf16 tensors
            if mode == 'bf16':      # a stride-2 layer writing LeakyReLU(result) as the copy (the codec's e2 -> block 1)
                w5 = g(rnd((5, 5, c, 64), 47, -0.05, 0.05), dev)
                y5, a5 = ops.conv2d(x, w5, None, stride=2, bf16_copy=True, copy_lrelu=True)
                assert torch.equal(y5, ops.conv2d(x, w5, None, stride=2))
                assert torch.equal(a5, ops.lrelu(y5).to(torch.bfloat16))
        finally:
            ops.set_compute('f32')
    ops.set_compute('bf16')
    try:
        from neural_imaging_amd import _lib
        wb = ops.weights_bf16(g(rnd((5, 5, c, c), 46), dev), 0)
        out = torch.empty_like(x)
        with pytest.raises(RuntimeError):           # the C ABI refuses shapes the fused epilogue does not serve
            _lib.call('nimg_conv2d_fwd_bf16_res', x.data_ptr(), c, wb.data_ptr(), None, out.data_ptr(), c, None, r.data_ptr(), None,
                      n, h, w, 5, 1, 2, 2, 0, h, w, 0, 0.2, 0, torch.cuda.current_stream().cuda_stream)
        wb3 = ops.weights_bf16(wk, 0)
        with pytest.raises(RuntimeError):           # ... and a call that asks for neither the skip sum nor the copy
            _lib.call('nimg_conv2d_fwd_bf16_res', x.data_ptr(), c, wb3.data_ptr(), None, out.data_ptr(), c, None, None, None,
                      n, h, w, 3, 1, 1, 1, 0, h, w, 0, 0.2, 0, torch.cuda.current_stream().cuda_stream)
    finally:
        ops.set_compute('f32')


def test_strided_dgrad_and_codec_small_ops(dev):
    from neural_imaging_amd import ops
    n, h, w, cin, cout, ks = 2, 16, 24, 8, 16, 5
    x = to64(rnd((n, h, w, cin), 1)).requires_grad_(True)
    wt = to64(rnd((ks, ks, cin, cout), 2, -0.2, 0.2))
    zc = T.conv2d(x, wt, None, 2, 'SAME')
    dz = rnd(tuple(zc.shape), 3)
    (zc * to64(dz)).sum().backward()
    dx = ops.conv2d_dgrad_strided2(g(dz, dev), g(wt.numpy(), dev), (h, w))
    assert_close(dx.cpu().numpy(), x.grad.numpy(), 1e-5, GRTOL, what='stride-2 dgrad (zero insertion)')
    a = rnd((1000,), 4)
    assert np.allclose(ops.affine(g(a, dev), 2.0, -1.0).cpu().numpy(), 2 * a - 1)
    assert np.allclose(ops.lrelu(g(a, dev)).cpu().numpy(), np.where(a > 0, a, 0.2 * a))
    t, y = rnd((2, 8, 8, 3), 5, 0, 1), rnd((2, 8, 8, 3), 6, 0, 1)
    lo, gr = ops.l2_loss(g(t, dev), g(y, dev), grad_scale=1.0)
    assert abs(float(lo.item()) - 0.5 * float(((t - y) ** 2).sum())) < 1e-4
    assert np.allclose(gr.cpu().numpy(), y - t, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------------
# throughput mode: bf16 operands / float32 accumulation (PSNR-level parity, not the 1e-4 contract)
@pytest.fixture()
def bf16_mode():
    from neural_imaging_amd import ops
    ops.set_compute('bf16')
    yield
    ops.set_compute('f32')


@pytest.mark.parametrize('shape', [(2, 8, 12, 64, 32), (5, 8, 8, 512, 256), (3, 16, 20, 24, 40), (2, 32, 32, 64, 32)])
def test_convt2x2_bf16_mode(dev, bf16_mode, shape):
    """Conv2DTranspose forward as four 1x1 MFMA products (bf16 operands): relative error at the bf16 level, and the
    phase (dy, dx) -> output position / kernel tap mapping must be exactly the float32 kernel's."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = shape
    x, wt, b = rnd((n, h, w, cin), 1), rnd((2, 2, cout, cin), 2, -0.3, 0.3), rnd((cout,), 3)
    y = ops.convt2x2(g(x, dev), g(wt, dev), g(b, dev)).cpu().numpy()
    ops.set_compute('f32')
    ref = ops.convt2x2(g(x, dev), g(wt, dev), g(b, dev)).cpu().numpy()
    ops.set_compute('bf16')
    err = np.abs(y - ref).max() / np.abs(ref).max()
    assert err < 1.5e-2, err
    # a one-hot tap: only phase (dy, dx) = (1, 0) may be non-zero (bias excluded)
    w1 = np.zeros_like(wt)
    w1[1, 0] = wt[1, 0]
    y1 = ops.convt2x2(g(x, dev), g(w1, dev), g(np.zeros_like(b), dev)).cpu().numpy()
    assert np.abs(y1[:, 0::2]).max() == 0 and np.abs(y1[:, 1::2, 1::2]).max() == 0 and np.abs(y1[:, 1::2, 0::2]).max() > 0


def test_pooled_gradient_kernels_bf16(dev, bf16_mode):
    """FAN conv1 backward from the POOLED gradient + arg-max bytes == un-pool pass followed by the ordinary weight /
    input gradient kernels, bit for bit (the staged bf16 operands are identical)."""
    from neural_imaging_amd import ops
    n, h, w = 3, 32, 48
    x, wt, b = rnd((n, h, w, 3), 1), rnd((5, 5, 3, 32), 2, -0.2, 0.2), rnd((32,), 3, -0.1, 0.1)
    xd, wd, bd = g(x, dev), g(wt, dev), g(b, dev)
    pooled, idx = ops.conv2d_pool(xd, wd, bd, act='leaky_relu')
    gp = g(rnd(tuple(pooled.shape), 4), dev)
    dz = ops.maxpool2_unpool(gp, idx, None, apply_mask=False)
    db_ref = torch.zeros(32, device=dev)
    dw_ref = ops.conv2d_wgrad(xd, dz, 5, db=db_ref)
    dx_ref = ops.conv2d_dgrad(dz, wd, (h, w))
    assert ops.pooled_backward_ok(3, 32, 5)
    db = torch.zeros(32, device=dev)
    dw = ops.conv2d_wgrad_pooled(xd, gp, idx, 5, db=db)
    dx = ops.conv2d_dgrad_pooled(gp, idx, wd)
    assert np.array_equal(dw.cpu().numpy(), dw_ref.cpu().numpy())
    assert np.array_equal(db.cpu().numpy(), db_ref.cpu().numpy())
    assert np.array_equal(dx.cpu().numpy(), dx_ref.cpu().numpy())
    # the pooled gradient stored as bf16: same operands after rounding => same weight / input gradients
    g16 = gp.to(torch.bfloat16)
    db2 = torch.zeros(32, device=dev)
    dw2 = ops.conv2d_wgrad_pooled(xd, g16, idx, 5, db=db2)
    dx2 = ops.conv2d_dgrad_pooled(g16, idx, wd)
    assert np.array_equal(dw2.cpu().numpy(), dw_ref.cpu().numpy())
    assert np.array_equal(dx2.cpu().numpy(), dx_ref.cpu().numpy())


def test_bf16_storage_is_bit_neutral(dev, bf16_mode):
    """Storing the un-pooled gradient in bf16 (throughput mode) changes no bit of what its consumers compute: they round
    their MFMA operands to bf16 anyway."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = 3, 32, 32, 32, 64
    x, wt = g(rnd((n, h, w, cin), 1), dev), g(rnd((5, 5, cin, cout), 2, -0.2, 0.2), dev)
    pooled, idx = ops.conv2d_pool(x, wt, g(rnd((cout,), 3), dev))
    gp = g(rnd(tuple(pooled.shape), 4), dev)
    dz32 = ops.maxpool2_unpool(gp, idx, None, apply_mask=False)
    dz16 = ops.maxpool2_unpool(gp, idx, None, apply_mask=False, out_bf16=True)
    assert dz16.dtype == torch.bfloat16 and torch.equal(dz16.float(), dz32.to(torch.bfloat16).float())
    db32, db16 = torch.zeros(cout, device=dev), torch.zeros(cout, device=dev)
    dw32 = ops.conv2d_wgrad(x, dz32, 5, db=db32)
    dw16 = ops.conv2d_wgrad(x, dz16, 5, db=db16)
    assert torch.equal(dw32, dw16)
    dx32 = ops.conv2d_dgrad(dz32, wt, (h, w), act_mask=x)
    dx16 = ops.conv2d_dgrad(dz16, wt, (h, w), act_mask=x)
    assert torch.equal(dx32, dx16)
    # the float32 bias sum sees the rounded values in the bf16 case: equal to rounding first
    db_ref = torch.zeros(cout, device=dev)
    ops.conv2d_wgrad(x, dz32.to(torch.bfloat16).float().contiguous(), 5, db=db_ref)
    assert torch.allclose(db16, db_ref, rtol=0, atol=1e-4 * float(db_ref.abs().max()))


BF16_CASES = [(2, 40, 72, 3, 0, 32, 5, 1), (2, 24, 24, 4, 0, 64, 3, 1), (2, 32, 32, 32, 0, 64, 5, 1), (2, 16, 16, 16, 16, 32, 3, 1), (5, 8, 8, 64, 0, 128, 3, 1),
              (2, 20, 24, 8, 0, 24, 3, 1), (2, 16, 24, 12, 0, 32, 3, 1), (3, 16, 16, 64, 0, 64, 1, 1), (2, 32, 32, 64, 0, 128, 5, 2)]


@pytest.mark.parametrize('case', BF16_CASES)
def test_conv2d_bf16_mode(dev, bf16_mode, case):
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout, ks, stride = case
    x = to64(rnd((n, h, w, c1 + c2), 1)).requires_grad_(True)
    wt = to64(rnd((ks, ks, c1 + c2, cout), 3, -0.2, 0.2)).requires_grad_(True)
    b = to64(rnd((cout,), 4)).requires_grad_(True)
    z = T.conv2d(x, wt, b, stride, 'SAME')
    dz = rnd(tuple(z.shape), 5)
    (z * to64(dz)).sum().backward()
    xg = g(x.detach().numpy(), dev)
    x1, x2 = (xg[..., :c1].contiguous(), xg[..., c1:].contiguous()) if c2 else (xg, None)
    out = ops.conv2d(x1, g(wt.detach().numpy(), dev), g(b.detach().numpy(), dev), x2=x2, stride=stride)
    assert_close(out.cpu().numpy(), z.detach().numpy(), 0.0, 1.5e-2, what='bf16 conv fwd {}'.format(case))
    dbf = torch.empty((cout,), device=dev)
    dw = ops.conv2d_wgrad(x1, g(dz, dev), ks, x2=x2, stride=stride, db=dbf)
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 0.0, 1.5e-2, what='bf16 wgrad {}'.format(case))
    assert_close(dbf.cpu().numpy(), b.grad.numpy(), 0.0, 1e-4, what='bias grad (f32 sums) {}'.format(case))
    if stride == 1:
        dx = ops.conv2d_dgrad(g(dz, dev), g(wt.detach().numpy(), dev), (h, w))
        assert_close(dx.cpu().numpy(), x.grad.numpy(), 0.0, 1.5e-2, what='bf16 dgrad {}'.format(case))


@pytest.mark.parametrize('shape', [(1, 64, 64, 64, 128), (1, 32, 32, 128, 256), (1, 128, 128, 32, 64), (2, 48, 40, 64, 64),
                                   (2, 24, 40, 32, 128)])
@pytest.mark.parametrize('stored_bf16', [False, True])
def test_dominant_conv5_at_bench_shapes(dev, bf16_mode, shape, stored_bf16):
    """The kernel family bench.py's roofline is quoted on - conv5_ring_kernel<128 / 64> (bf16-stored tensors, Cout % 64 == 0),
    conv_fwd_bf16_kernel<5,1,16,16,1,64,...> (float32 tensors) and conv_wgrad_bf16_kernel<5,..> - at the layer shapes of the
    bench (FAN conv2: 32 -> 64 @ 128x128, conv3: 64 -> 128 @ 64x64, conv4: 128 -> 256 @ 32x32; 2, 4 and 8 channel chunks) and
    at two ragged sizes (partial 32x16 / 16x16 tiles), forward (plain and with the fused LeakyReLU + pool epilogue), input
    gradient and weight gradient against the float64 oracle, with float32 tensors and with the bf16-stored tensors the
    throughput-mode FAN feeds it."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = shape
    x_np, dz_np = rnd((n, h, w, cin), 1), rnd((n, h, w, cout), 5)
    if stored_bf16:      # the tensors live in HBM as bf16: the oracle sees the same rounded values
        x_np, dz_np = _bf16_round(x_np).numpy().astype(np.float32), _bf16_round(dz_np).numpy().astype(np.float32)
    x = to64(x_np).requires_grad_(True)
    wt = to64(rnd((5, 5, cin, cout), 3, -0.05, 0.05)).requires_grad_(True)
    b = to64(rnd((cout,), 4))
    z = T.conv2d(x, wt, b, 1, 'SAME')
    (z * to64(dz_np)).sum().backward()
    dt = torch.bfloat16 if stored_bf16 else torch.float32
    xg, dzg = g(x_np, dev).to(dt), g(dz_np, dev).to(dt)
    wg, bg = g(wt.detach().numpy(), dev), g(b.numpy(), dev)
    out = ops.conv2d(xg, wg, bg)
    assert_close(out.cpu().numpy(), z.detach().numpy(), 0.0, 1.5e-2, what='fwd')
    pooled, idx = ops.conv2d_pool(xg, wg, bg, out_bf16=stored_bf16)
    act = T.leaky_relu(z.detach())
    assert_close(pooled.float().cpu().numpy(), T.max_pool2(act).numpy(), 0.0, 1.5e-2, what='fwd + lrelu + pool')
    win = act.numpy().reshape(n, h // 2, 2, w // 2, 2, cout).transpose(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, cout, 4)
    srt = np.sort(win, axis=-1)
    clear = (srt[..., 3] - srt[..., 2]) > 2e-2 * np.abs(act.numpy()).max()
    assert clear.mean() > 0.7 and np.array_equal(idx.cpu().numpy()[clear], win.argmax(axis=-1)[clear])
    dx = ops.conv2d_dgrad(dzg, wg, (h, w), out_bf16=stored_bf16)
    assert_close(dx.float().cpu().numpy(), x.grad.numpy(), 0.0, 1.5e-2, what='dgrad')
    dbf = torch.empty((cout,), device=dev)
    dw = ops.conv2d_wgrad(xg, dzg, 5, db=dbf)
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 0.0, 1.5e-2, what='wgrad')
    assert_close(dbf.cpu().numpy(), dz_np.astype(np.float64).sum(axis=(0, 1, 2)), 0.0, 1e-4, what='bias grad')


@pytest.mark.parametrize('shape', [(2, 32, 32, 32, 64), (1, 64, 64, 64, 128), (3, 16, 48, 128, 256)])
def test_unpool_folded_into_conv5_backward(dev, bf16_mode, shape):
    """nimg_conv2d_fwd_bf16_unpool / nimg_conv2d_wgrad_bf16_unpool: the 5x5 input- and weight-gradient kernels reading the pooled
    gradient + arg-max bytes are bit-identical to un-pooling first (nimg_maxpool2_unpool_ex) and running the plain kernels."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = shape
    x = g(rnd((n, h, w, cin), 1), dev).to(torch.bfloat16)
    gp = g(rnd((n, h // 2, w // 2, cout), 2), dev).to(torch.bfloat16)
    idx = torch.from_numpy(np.random.default_rng(3).integers(0, 4, size=(n, h // 2, w // 2, cout)).astype(np.uint8)).to(dev)
    wt = g(rnd((5, 5, cin, cout), 4, -0.05, 0.05), dev)
    mask = g(rnd((n, h, w, cin), 5), dev).to(torch.bfloat16)
    assert ops.unpool_fold_ok(x, gp, cin, cout, 5)
    dz = ops.maxpool2_unpool(gp, idx, None, apply_mask=False, out_bf16=True)
    for out_bf16, am in ((False, None), (True, mask)):
        ref = ops.conv2d_dgrad(dz, wt, (h, w), act_mask=am, out_bf16=out_bf16)
        was = ops.SPARSE_DGRAD
        try:
            ops.SPARSE_DGRAD = False
            got = ops.conv2d_dgrad_unpool(gp, idx, wt, act_mask=am, out_bf16=out_bf16)
            assert torch.equal(ref, got), 'input gradient'
            # the structured-sparsity form (csrc/dgrad5s.hip): the same bf16 products, another summation order
            ops.SPARSE_DGRAD = True
            sp = ops.conv2d_dgrad_unpool(gp, idx, wt, act_mask=am, out_bf16=out_bf16)
        finally:
            ops.SPARSE_DGRAD = was
        tol = (8e-3 if out_bf16 else 2e-5) * float(ref.float().abs().max())
        assert float((sp.float() - ref.float()).abs().max()) <= tol, 'input gradient, sparse form'
    dw_ref, db_ref = torch.empty_like(wt), torch.empty((cout,), device=dev)
    ops.conv2d_wgrad(x, dz, 5, dw=dw_ref, db=db_ref)
    dw, db = torch.empty_like(wt), torch.empty((cout,), device=dev)
    ops.conv2d_wgrad_unpool(x, gp, idx, 5, dw, db=db)
    # the pooled form runs the all-taps kernel (csrc/wgrad5.hip) where its shape rules allow: same products, another summation
    # order (float32 sums of exact bf16 x bf16 products) - test_wgrad5_alltaps_vs_oracle holds it to the float64 oracle
    assert torch.allclose(dw_ref, dw, rtol=0, atol=2e-5 * float(dw_ref.abs().max())), 'weight gradient'
    assert torch.allclose(db_ref, db, rtol=0, atol=2e-5 * float(gp.float().abs().sum(dim=(0, 1, 2)).max())), 'bias gradient'


@pytest.mark.parametrize('shape', [(2, 128, 128, 32, 64), (3, 64, 64, 64, 128), (2, 32, 32, 128, 256), (1, 8, 16, 32, 64),
                                   (3, 24, 40, 64, 72), (1, 36, 34, 32, 8)])
def test_dgrad5_sparse_vs_oracle(dev, bf16_mode, shape):
    """csrc/dgrad5s.hip (v_smfmac_f32_32x32x32_bf16: the pooled gradient as the compressed operand, the arg-max byte as its index):
    input gradient of a fused 5x5 conv + pool layer at the FAN's layer shapes, an image smaller than one 16 x 16 pooled tile, sizes
    the tiles do not divide and channel counts off the usual multiples, against float64 autograd through the convolution on
    the same rounded values - with and without the LeakyReLU' mask of the layer below, float32 and bf16 outputs."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = shape
    gp_np = _bf16_round(rnd((n, h // 2, w // 2, cout), 12)).numpy().astype(np.float32)
    idx_np = np.random.default_rng(13).integers(0, 4, size=(n, h // 2, w // 2, cout)).astype(np.uint8)
    dz_np = np.zeros((n, h, w, cout), np.float32)
    for pos in range(4):
        dz_np[:, pos >> 1::2, pos & 1::2, :] = np.where(idx_np == pos, gp_np, 0.0)
    wt_np = rnd((5, 5, cin, cout), 14, -0.05, 0.05)
    x = to64(np.zeros((n, h, w, cin))).requires_grad_(True)
    (T.conv2d(x, _bf16_round(wt_np), None, 1, 'SAME') * to64(dz_np)).sum().backward()
    ref = x.grad.numpy()
    mask_np = rnd((n, h, w, cin), 15)
    gg, ig = g(gp_np, dev).to(torch.bfloat16), torch.from_numpy(idx_np).to(dev)
    was = ops.SPARSE_DGRAD
    ops.SPARSE_DGRAD = True                      # off by default (at parity with the ring kernels): the kernel is kept and held to the oracle
    try:
        got = ops.conv2d_dgrad_unpool(gg, ig, g(wt_np, dev))
        gm = ops.conv2d_dgrad_unpool(gg, ig, g(wt_np, dev), act_mask=g(mask_np, dev).to(torch.bfloat16), out_bf16=True)
    finally:
        ops.SPARSE_DGRAD = was
    assert_close(got.cpu().numpy(), ref, 0.0, 2e-5, what='sparse dgrad')
    refm = ref * np.where(_bf16_round(mask_np).numpy() > 0, 1.0, 0.2)
    assert gm.dtype == torch.bfloat16
    assert_close(gm.float().cpu().numpy(), refm, 0.0, 8e-3, what='sparse dgrad, masked, bf16 out')


@pytest.mark.parametrize('shape', [(4, 128, 128, 32, 64), (5, 64, 64, 64, 128), (7, 32, 32, 128, 256), (1, 8, 16, 32, 64),
                                   (3, 24, 32, 64, 192)])
def test_wgrad5_alltaps_vs_oracle(dev, bf16_mode, shape):
    """csrc/wgrad5.hip (all 25 taps in one wave, v_mfma_f32_16x16x32_bf16, shifted register windows, double-buffered tiles): weight
    and bias gradient of the FAN's conv2 / conv3 / conv4 from (bf16 input, pooled bf16 gradient, arg-max bytes) at the bench's
    layer shapes (32 -> 64 @ 128x128, 64 -> 128 @ 64x64, 128 -> 256 @ 32x32; batch sizes that do not divide over the splits), a
    single-tile image and a 16-row-indivisible one (8-row tiles), against the float64 oracle on the same rounded values."""
    from neural_imaging_amd import ops
    n, h, w, cin, cout = shape
    x_np = _bf16_round(rnd((n, h, w, cin), 11)).numpy().astype(np.float32)
    gp_np = _bf16_round(rnd((n, h // 2, w // 2, cout), 12)).numpy().astype(np.float32)
    idx_np = np.random.default_rng(13).integers(0, 4, size=(n, h // 2, w // 2, cout)).astype(np.uint8)
    dz_np = np.zeros((n, h, w, cout), np.float32)
    for pos in range(4):
        dz_np[:, pos >> 1::2, pos & 1::2, :] = np.where(idx_np == pos, gp_np, 0.0)
    x = to64(x_np)
    wt = to64(np.zeros((5, 5, cin, cout))).requires_grad_(True)
    z = T.conv2d(x, wt, None, 1, 'SAME')
    (z * to64(dz_np)).sum().backward()
    xg, gg = g(x_np, dev).to(torch.bfloat16), g(gp_np, dev).to(torch.bfloat16)
    ig = torch.from_numpy(idx_np).to(dev)
    assert ops.unpool_fold_ok(xg, gg, cin, cout, 5)
    dw, db = torch.full((5, 5, cin, cout), 7.0, device=dev), torch.full((cout,), 7.0, device=dev)
    ops.conv2d_wgrad_unpool(xg, gg, ig, 5, dw, db=db)
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 0.0, 2e-5, what='wgrad')
    assert_close(db.cpu().numpy(), dz_np.astype(np.float64).sum(axis=(0, 1, 2)), 0.0, 2e-5, what='bias grad')


@pytest.mark.parametrize('shape', [(3, 128, 128, 32, 0, 32), (2, 128, 128, 32, 32, 32), (3, 64, 64, 32, 0, 64),
                                   (3, 64, 64, 64, 64, 64), (5, 32, 32, 128, 128, 128), (7, 16, 16, 256, 0, 256),
                                   (2, 24, 32, 64, 0, 32), (1, 8, 16, 32, 0, 128), (3, 16, 16, 512, 0, 256)])
def test_wgrad3_alltaps_vs_oracle(dev, bf16_mode, shape):
    """csrc/wgrad3.hip (all 9 taps in one wave, v_mfma_f32_16x16x32_bf16, double-buffered tiles with two tiles of loads in
    flight, row groups folded through LDS): weight and bias gradient of the UNet's 3x3 layers from bf16-stored tensors at its
    layer shapes - level 1 (Cout 32, 16-row tiles, four row groups), the two-tensor decoder inputs, levels 2 - 4, an image the
    16-row tiles do not divide, a single-tile image - against the float64 oracle on the same rounded values."""
    from neural_imaging_amd import ops
    n, h, w, c1, c2, cout = shape
    x1 = _bf16_round(rnd((n, h, w, c1), 31)).numpy().astype(np.float32)
    x2 = _bf16_round(rnd((n, h, w, c2), 32)).numpy().astype(np.float32) if c2 else None
    dz = _bf16_round(rnd((n, h, w, cout), 33)).numpy().astype(np.float32)
    xin = np.concatenate([x1, x2], axis=-1) if c2 else x1
    wt = to64(np.zeros((3, 3, c1 + c2, cout))).requires_grad_(True)
    (T.conv2d(to64(xin), wt, None, 1, 'SAME') * to64(dz)).sum().backward()
    bf = torch.bfloat16
    dw, db = torch.full((3, 3, c1 + c2, cout), 7.0, device=dev), torch.full((cout,), 7.0, device=dev)
    ops.conv2d_wgrad(g(x1, dev).to(bf), g(dz, dev).to(bf), 3, x2=g(x2, dev).to(bf) if c2 else None, dw=dw, db=db)
    assert_close(dw.cpu().numpy(), wt.grad.numpy(), 0.0, 2e-5, what='wgrad')
    assert_close(db.cpu().numpy(), dz.astype(np.float64).sum(axis=(0, 1, 2)), 0.0, 2e-5, what='bias grad')


def test_bf16_stored_unet_ops(dev, bf16_mode):
    """The throughput-mode entry points on bf16-STORED tensors (UNet activations / gradients): two-tensor inputs and outputs,
    the 2x2 / stride-2 forms behind Conv2DTranspose, max-pool forward / backward, the bias gradient, the 4-channel first
    convolution with a bf16 output.  Each equals the same op on float32 copies of the same (rounded) values, rounded once."""
    from neural_imaging_amd import ops
    bf = torch.bfloat16
    n, h, w, c = 2, 16, 24, 32
    x1, x2 = g(rnd((n, h, w, c), 1), dev).to(bf), g(rnd((n, h, w, c), 2), dev).to(bf)
    wt = g(rnd((3, 3, 2 * c, c), 3, -0.05, 0.05), dev)
    b = g(rnd((c,), 4), dev)
    y16 = ops.conv2d(x1, wt, b, x2=x2, act='leaky_relu', out_bf16=True)
    y32 = ops.conv2d(x1.float(), wt, b, x2=x2.float(), act='leaky_relu')
    assert y16.dtype == bf and torch.equal(y16, y32.to(bf)), 'two-input forward'
    dz = g(rnd((n, h, w, c), 5), dev).to(bf)
    d1, d2 = torch.empty_like(x1), torch.empty_like(x2)
    ops.conv2d_dgrad(dz, wt, (h, w), out=d1, out2=d2)
    e1, e2 = torch.empty((n, h, w, c), device=dev), torch.empty((n, h, w, c), device=dev)
    ops.conv2d_dgrad(dz.float(), wt, (h, w), out=e1, out2=e2)
    assert torch.equal(d1, e1.to(bf)) and torch.equal(d2, e2.to(bf)), 'two-output input gradient'
    dw16, db16 = torch.empty_like(wt), torch.empty((c,), device=dev)
    ops.conv2d_wgrad(x1, dz, 3, x2=x2, dw=dw16, db=db16)
    dw32, db32 = torch.empty_like(wt), torch.empty((c,), device=dev)
    ops.conv2d_wgrad(x1.float(), dz.float(), 3, x2=x2.float(), dw=dw32, db=db32)
    assert torch.equal(dw16, dw32) and torch.allclose(db16, db32, rtol=0, atol=1e-5 * float(db32.abs().max())), 'two-input wgrad'
    # Conv2DTranspose: forward, input gradient (2x2 / stride 2 with the LeakyReLU' mask), weight gradient, bias gradient
    wt2 = g(rnd((2, 2, c, 2 * c), 6, -0.05, 0.05), dev)                     # (2,2,Cout,Cin)
    xin = g(rnd((n, h // 2, w // 2, 2 * c), 7), dev).to(bf)
    up16 = ops.convt2x2(xin, wt2, b, out_bf16=True)
    up32 = ops.convt2x2(xin.float(), wt2, b)
    assert up16.dtype == bf and torch.equal(up16, up32.to(bf)), 'transposed convolution'
    g16 = ops.convt2x2_dgrad(dz, wt2, act_mask=xin, out_bf16=True)
    g32 = ops.convt2x2_dgrad(dz.float(), wt2, act_mask=xin.float())
    assert g16.dtype == bf and torch.equal(g16, g32.to(bf)), 'transposed convolution: input gradient'
    assert torch.equal(ops.convt2x2_wgrad(xin, dz), ops.convt2x2_wgrad(xin.float(), dz.float())), 'transposed convolution: wgrad'
    assert torch.allclose(ops.bias_grad(dz), ops.bias_grad(dz.float()), rtol=0, atol=1e-5 * float(dz.float().abs().sum())), 'bias'
    # pooling
    p16 = ops.maxpool2(x1)
    assert p16.dtype == bf and torch.equal(p16, ops.maxpool2(x1.float()).to(bf)), 'max-pool'
    dp = g(rnd((n, h // 2, w // 2, c), 8), dev).to(bf)
    q16 = ops.maxpool2_bwd(dp, x1, add=x2, apply_mask=True)
    q32 = ops.maxpool2_bwd(dp.float(), x1.float(), add=x2.float(), apply_mask=True)
    assert q16.dtype == bf and torch.equal(q16, q32.to(bf)), 'max-pool backward'
    # first convolution of the UNet: 4 float32 channels in, bf16 out
    raw = g(rnd((n, h, w, 4), 9), dev)
    w4 = g(rnd((3, 3, 4, c), 10, -0.2, 0.2), dev)
    f16 = ops.conv2d(raw, w4, b, act='leaky_relu', out_bf16=True)
    assert f16.dtype == bf and torch.equal(f16, ops.conv2d(raw, w4, b, act='leaky_relu').to(bf)), 'first convolution'


def test_fan_conv1_input_gradient_bf16(dev, bf16_mode):
    """kx-folded MFMA input gradient of the FAN's first convolution (5x5, 3 <- 32), incl. partial tiles."""
    from neural_imaging_amd import ops
    for (n, h, w) in [(2, 32, 56), (1, 48, 40), (3, 16, 16)]:
        x = to64(rnd((n, h, w, 3), 1)).requires_grad_(True)
        wt = to64(rnd((5, 5, 3, 32), 3, -0.2, 0.2))
        z = T.conv2d(x, wt, None, 1, 'SAME')
        dz = rnd(tuple(z.shape), 5)
        (z * to64(dz)).sum().backward()
        dx = ops.conv2d_dgrad(g(dz, dev), g(wt.numpy(), dev), (h, w))
        assert_close(dx.cpu().numpy(), x.grad.numpy(), 0.0, 1.5e-2, what='fewin dgrad {}'.format((n, h, w)))


@pytest.mark.parametrize('name', ['awgn', 'gamma', 'median3', 'median5'])
def test_more_manipulations_fwd_bwd(dev, name):
    """awgn / gamma / median (helpers/tf_helpers.py:79-110); awgn with injected noise (tf.random.normal is not
    reproducible)."""
    from neural_imaging_amd.helpers import tf_helpers as th
    x_np = (0.05 + 0.9 * np.random.default_rng(3).random((2, 20, 24, 3))).astype(np.float32)   # no ties, inside (0,1)
    x = to64(x_np).requires_grad_(True)
    noise = rnd(x_np.shape, 9)
    if name == 'awgn':
        op, ref = th.Awgn(), om.manipulation_awgn(x, 5.1 / 255, to64(noise))
        y, ctx = op.forward(g(x_np, dev), 5.1, training=True, noise=g(noise, dev))
    elif name == 'gamma':
        op, ref = th.Gamma(), om.manipulation_gamma(x, 3.0)
        y, ctx = op.forward(g(x_np, dev), 3.0, training=True)
    else:
        k = int(name[-1])
        op, ref = th.Median(), om.manipulation_median(x, k)
        y, ctx = op.forward(g(x_np, dev), k, training=True)
    dy = rnd(tuple(ref.shape), 4)
    (ref * to64(dy)).sum().backward()
    # hard rounding inside awgn/gamma: a float32/float64 tie may flip a value by 1/255 at isolated elements
    d = np.abs(y.cpu().numpy() - ref.detach().numpy())
    assert np.mean(d > 1e-4) < 2e-3 and d.max() < 0.02, (np.mean(d > 1e-4), d.max())
    dx = op.backward(ctx, g(dy, dev)).cpu().numpy()
    e = np.abs(dx - x.grad.numpy())
    assert np.mean(e > 2e-3 * np.abs(x.grad.numpy()).max()) < 5e-3, np.mean(e > 2e-3 * np.abs(x.grad.numpy()).max())


@pytest.mark.parametrize('count', [0, 5, 4096 + 3, 3 * 64 * 64 * 3])
def test_classic_isp_pointwise(dev, count):
    """nimg_isp_residual_*, nimg_sigmoid_*, nimg_gamma_ste_* (ClassicISP, models/pipelines.py:416-453,
    models/layers.py:252-255) against float64 autograd, incl. the empty and the non-multiple-of-4 stream."""
    from neural_imaging_amd import ops
    x, f, dy = rnd((count,), 1) * 0.8 + 0.4, rnd((count,), 2), rnd((count,), 3)
    alpha = np.array([0.37], np.float32)
    xt, ft, at = to64(x).requires_grad_(True), to64(f).requires_grad_(True), to64(alpha).requires_grad_(True)
    ste = lambda t, lo, hi: t + (torch.clamp(t, lo, hi) - t).detach()
    y_ref = ste(xt - at * ft, 0.0, 1.0)
    y = ops.isp_residual(g(x, dev), g(f, dev), g(alpha, dev))
    assert_close(y.cpu().numpy(), y_ref.detach().numpy(), 1e-6, what='residual')
    y0 = ops.isp_residual(g(x, dev), None, g(alpha, dev))
    assert np.array_equal(y0.cpu().numpy(), np.clip(x, 0, 1))
    dalpha = torch.full((1,), 7.0, device=dev)
    df = ops.isp_residual_bwd(g(dy, dev), g(f, dev), g(alpha, dev), dalpha)
    if count:
        gf, ga = torch.autograd.grad((y_ref * to64(dy)).sum(), [ft, at])
        assert_close(df.cpu().numpy(), gf.numpy(), 1e-6, what='d f')
        assert_close(dalpha.cpu().numpy(), ga.numpy(), 1e-5, 1e-5, what='d alpha')
        d2 = dalpha.clone()
        ops.isp_residual_bwd(g(dy, dev), g(f, dev), g(alpha, dev), d2, accumulate=True)
        assert_close(d2.cpu().numpy(), 2 * ga.numpy(), 1e-5, 1e-5, what='d alpha accumulated')
    else:
        assert float(dalpha.item()) == 0.0
    # sigmoid
    s_ref = torch.sigmoid(ft * 3)
    sg = ops.sigmoid(g(f * 3, dev))
    assert_close(sg.cpu().numpy(), s_ref.detach().numpy(), 1e-6, what='sigmoid')
    if count:
        gs, = torch.autograd.grad((s_ref * to64(dy)).sum(), [ft])
        assert_close(3 * ops.sigmoid_bwd(g(dy, dev), sg).cpu().numpy(), gs.numpy(), 1e-5, what='d sigmoid')
    # gamma stage: values below 1/255 and above 1 take the clipped value but keep a gradient
    v = (rnd((count,), 4) * 0.7 + 0.4).astype(np.float32)
    vt = to64(v).requires_grad_(True)
    g_ref = torch.pow(ste(vt, 1.0 / 255, 1.0), 1 / 2.2)
    gy = ops.gamma_ste(g(v, dev))
    assert_close(gy.cpu().numpy(), g_ref.detach().numpy(), 2e-6, what='gamma')
    if count:
        gg, = torch.autograd.grad((g_ref * to64(dy)).sum(), [vt])
        assert_close(ops.gamma_ste_bwd(g(v, dev), g(dy, dev)).cpu().numpy(), gg.numpy(), 1e-5, what='d gamma')


@pytest.mark.parametrize('metric,shape', [('L1', (2, 16, 16, 3)), ('L1', (1, 7, 5, 3)), ('SSIM', (3, 32, 40, 3)),
                                          ('SSIM', (1, 11, 11, 3)), ('SSIM', (2, 17, 12, 1)), ('L2', (2, 16, 16, 3)),
                                          ('MS-SSIM', (2, 176, 192, 3)), ('MS-SSIM', (1, 256, 256, 1))])
def test_image_losses_with_gradient(dev, metric, shape):
    """The NIP training losses (helpers/tf_helpers.py:31-40 via models/pipelines.py:53-63): value, gradient w.r.t. the
    developed image, gradient accumulation with a scale (the workflow's lambda_nip term)."""
    from neural_imaging_amd import ops
    n, h, w, c = shape
    t = natural_images(n, h, w, seed=5)[..., :c].copy()
    y = np.clip(t + 0.08 * rnd(t.shape, 6), 0, 1).astype(np.float32)
    y[0, 0, 0, 0] = t[0, 0, 0, 0]                            # an exact tie: tf.abs has a zero gradient there
    yt = to64(y).requires_grad_(True)
    ref = T.IMAGE_LOSSES[metric](yt, to64(t))
    gref, = torch.autograd.grad(ref, [yt])
    fn = ops.IMAGE_LOSSES[metric]
    loss, grad = fn(g(y, dev), g(t, dev), grad_scale=1.0)
    assert abs(float(loss.item()) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    assert_close(grad.cpu().numpy(), gref.numpy(), 1e-7, 1e-5, what=metric + ' gradient')
    base = rnd(t.shape, 7)
    acc = g(base, dev)
    loss2, out = fn(g(y, dev), g(t, dev), grad_scale=0.25, grad_out=acc, accumulate=True)
    assert out is acc and float(loss2.item()) == float(loss.item())
    assert_close(acc.cpu().numpy(), base + 0.25 * gref.numpy(), 1e-6, 1e-5, what=metric + ' accumulated gradient')
    assert fn(g(y, dev), g(t, dev))[1] is None
    if metric == 'SSIM':
        with pytest.raises(ValueError):
            ops.ssim_loss(g(y[:, :10], dev), g(t[:, :10], dev))
    if metric == 'MS-SSIM':
        with pytest.raises(ValueError):
            ops.msssim_loss(g(y[:, :168], dev), g(t[:, :168], dev))


def _feed_images(n, h, w, seed):
    rng = np.random.RandomState(seed)
    rgb = np.zeros((n, h, w, 3), np.uint8)
    for i in range(n):
        base = np.full((h, w, 3), 40.0 + 25 * i)
        base[h // 4:h // 2, w // 3:] += 80 * rng.uniform(-1, 1, (h // 2 - h // 4, w - w // 3, 3))
        base[:, :w // 4] += 15 * np.sin(np.arange(w // 4) / 2.0)[None, :, None]
        rgb[i] = np.clip(base + rng.normal(0, 2, (h, w, 3)), 0, 255)
    rgb[n - 1] = 77                                           # a perfectly flat image: variance exactly 0
    raw = rng.randint(0, 65536, (n, h // 2, w // 2, 4)).astype(np.uint16)
    return raw, rgb


@pytest.mark.parametrize('discard', [None, 'flat', 'flat-aggressive', 'dark-n-textured'])
@pytest.mark.parametrize('patch,attempts,max_attempts', [(32, 12, 5), (64, 30, 25), (96, 4, 4)])
def test_device_data_feed_kernels(dev, discard, patch, attempts, max_attempts):
    """nimg_patch_stats / _select / _gather (helpers/dataset.py:89-131, helpers/loading.py:132-211) against the oracle that
    is pinned on the reference's own sample_patch: patch moments, the discard policy over a given candidate list (same
    corner, same number of candidates consumed), and the cut batch bit for bit."""
    from oracle import datafeed as odf
    from neural_imaging_amd import ops
    raw, rgb = _feed_images(6, 96, 128, 9)
    rng = np.random.RandomState(patch + attempts)
    b = 9
    image_idx = rng.randint(0, 6, b).astype(np.int32)
    image_idx[-1] = 5
    cand = np.stack([2 * (rng.randint(0, max(128 - patch, 1), (b, attempts)) // 2),
                     2 * (rng.randint(0, max(96 - patch, 1), (b, attempts)) // 2)], axis=2).astype(np.int32)
    uni = rng.uniform(size=(b, attempts)).astype(np.float32)
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_raw = torch.from_numpy(raw.view(np.int16)).to(dev)
    d_idx, d_cand, d_uni = torch.from_numpy(image_idx).to(dev), torch.from_numpy(cand).to(dev), torch.from_numpy(uni).to(dev)
    var, mean = ops.patch_stats(d_rgb, d_idx, d_cand, patch)
    ref = np.array([[odf.patch_stats(rgb[image_idx[i]], cand[i, k, 0], cand[i, k, 1], patch) for k in range(attempts)]
                    for i in range(b)])
    assert np.abs(var.cpu().numpy() - ref[..., 0]).max() < 1e-13 and np.abs(mean.cpu().numpy() - ref[..., 1]).max() < 1e-13
    # flat image: exactly zero (exact integer moments).  np.var of a constant patch / 255 is a residue of ~1e-34 at most levels,
    # within the 1e-13 above; at level 77 the mean 0.302 < 0.35 makes both sides reject the patch in 'dark-n-textured' anyway
    # (levels where they differ: tests/test_gpu_operands_exact.py::test_flat_patches_in_dark_n_textured)
    assert (var.cpu().numpy()[-1] == 0).all()
    xy, used = ops.patch_select(d_cand, d_uni, var if discard else None, mean if discard else None, discard, max_attempts)
    want = [odf.select(rgb[image_idx[i]], [tuple(c) for c in cand[i]], uni[i], patch, discard, max_attempts)
            for i in range(b)]
    assert xy.cpu().numpy().tolist() == [list(w[0]) for w in want]
    assert used.cpu().numpy().tolist() == [w[1] for w in want]
    x, y = ops.patch_gather(d_raw, d_rgb, d_idx, xy, patch)
    xr, yr = odf.cut_batch(raw, rgb, image_idx, [w[0] for w in want], patch)
    assert x.dtype == torch.float32 and np.array_equal(x.cpu().numpy(), xr) and np.array_equal(y.cpu().numpy(), yr)
    only_y = ops.patch_gather(None, d_rgb, d_idx, xy, patch)
    assert only_y[0] is None and np.array_equal(only_y[1].cpu().numpy(), yr)
    only_x = ops.patch_gather(d_raw, None, d_idx, xy, patch)
    assert only_x[1] is None and np.array_equal(only_x[0].cpu().numpy(), xr)
    with pytest.raises(RuntimeError):
        ops.patch_stats(d_rgb, d_idx, d_cand, 200)
    with pytest.raises(TypeError):
        ops.patch_gather(d_raw.to(torch.int32), d_rgb, d_idx, xy, patch)


def test_device_dataset(dev):
    """helpers/dataset.DeviceDataset: the host sampler reproduces Dataset.next_training_batch bit for bit (same numpy RNG
    stream); the device sampler is deterministic per seed, stays on the Bayer grid inside the image and returns exactly
    the crop at the corners it chose; validation batches equal the host's; batches feed a pipeline directly."""
    from neural_imaging_amd.helpers import dataset
    from neural_imaging_amd.models import pipelines
    raw, rgb = _feed_images(8, 96, 128, 21)
    host = dataset.Dataset.from_arrays({'x': raw[:6], 'y': rgb[:6]}, {'x': raw[6:, :16, :16], 'y': rgb[6:, :32, :32]})
    feed = dataset.DeviceDataset(host, device=dev, sampler='host')
    for discard in (None, 'flat', 'flat-aggressive', 'dark-n-textured'):
        np.random.seed(4)
        xh, yh = host.next_training_batch(1, 3, 48, discard, max_attempts=7)
        np.random.seed(4)
        xd, yd = feed.next_training_batch(1, 3, 48, discard, max_attempts=7)
        assert np.array_equal(xd.numpy(), xh) and np.array_equal(yd.numpy(), yh)
    xv, yv = feed.next_validation_batch(0, 2)
    xvh, yvh = host.next_validation_batch(0, 2)
    assert np.array_equal(xv.numpy(), xvh) and np.array_equal(yv.numpy(), yvh)
    assert feed.count_training == 6 and feed.rgb_patch_size == 32 and 'raw+rgb' in feed.summary()
    a, b_ = dataset.DeviceDataset(host, device=dev, seed=5), dataset.DeviceDataset(host, device=dev, seed=5)
    c = dataset.DeviceDataset(host, device=dev, seed=6)
    seen = []
    for discard in (None, 'flat', 'flat-aggressive', 'dark-n-textured'):
        xa, ya = a.next_training_batch(0, 6, 64, discard)
        xb, yb = b_.next_training_batch(0, 6, 64, discard)
        c.next_training_batch(0, 6, 64, discard)
        xy = a.last_xy.cpu().numpy()
        assert np.array_equal(xy, b_.last_xy.cpu().numpy()) and np.array_equal(ya.numpy(), yb.numpy())
        assert (xy % 2 == 0).all() and (xy >= 0).all() and (xy[:, 0] <= 128 - 64).all() and (xy[:, 1] <= 96 - 64).all()
        for i in range(6):
            assert np.array_equal(ya.numpy()[i], (rgb[i, xy[i, 1]:xy[i, 1] + 64, xy[i, 0]:xy[i, 0] + 64] / 255.0).astype(np.float32))
            assert np.array_equal(xa.numpy()[i], (raw[i, xy[i, 1] // 2:xy[i, 1] // 2 + 32, xy[i, 0] // 2:xy[i, 0] // 2 + 32]
                                                  / 65535.0).astype(np.float32))
        seen.append((xy, c.last_xy.cpu().numpy()))
    assert any(not np.array_equal(p, q) for p, q in seen)      # another seed, other corners
    net = pipelines.INet(patch_size=32, device=dev)
    xa, ya = a.next_training_batch(0, 6, 64, 'flat')
    assert np.isfinite(float(net.training_step(xa, ya, learning_rate=1e-3)))
    with pytest.raises(ValueError):
        a.next_training_batch(0, 6, 63)
    with pytest.raises(ValueError):
        a.next_training_batch(1, 6, 64)



def test_torch_library_custom_ops(dev):
    """neural_imaging_amd.torch_ops: the C-ABI kernels as dispatcher-visible PyTorch custom ops (namespace nimg) with autograd -
    dJPEG and Conv2D gradients through torch.autograd equal the explicit backward entry points."""
    from neural_imaging_amd import ops, torch_ops
    x = g(natural_images(2, 32, 32, seed=3), dev).requires_grad_(True)
    q = ops.qtables_device(75, dev)
    y = torch.ops.nimg.djpeg(x, q, 'soft')
    gy = g(rnd((2, 32, 32, 3), 2), dev)
    y.backward(gy)
    y_ref, mask, _, _ = ops.djpeg_fwd(x.detach(), q, 'soft', want_mask=True)
    assert torch.equal(y.detach(), y_ref) and torch.equal(x.grad, ops.djpeg_bwd(x.detach(), gy, mask, q, 'soft'))
    a = g(rnd((2, 16, 16, 8), 4), dev).requires_grad_(True)
    w = g(rnd((3, 3, 8, 16), 5, -0.2, 0.2), dev).requires_grad_(True)
    b = g(rnd((16,), 6), dev).requires_grad_(True)
    z = torch_ops.conv2d(a, w, b, 1, 'leaky_relu')
    gz = g(rnd((2, 16, 16, 16), 7), dev)
    z.backward(gz)
    at, wt, bt = to64(a.detach().cpu().numpy()).requires_grad_(True), to64(w.detach().cpu().numpy()).requires_grad_(True), \
        to64(b.detach().cpu().numpy()).requires_grad_(True)
    zr = T.leaky_relu(T.conv2d(at, wt, bt))
    (zr * to64(gz.cpu().numpy())).sum().backward()
    assert_close(z.detach().cpu().numpy(), zr.detach().numpy(), 1e-4, what='custom-op conv fwd')
    assert_close(a.grad.cpu().numpy(), at.grad.numpy(), 1e-4, GRTOL, what='custom-op conv d input')
    assert_close(w.grad.cpu().numpy(), wt.grad.numpy(), 1e-4, GRTOL, what='custom-op conv d kernel')
    assert_close(b.grad.cpu().numpy(), bt.grad.numpy(), 1e-4, GRTOL, what='custom-op conv d bias')
    with pytest.raises(NotImplementedError):
        torch.ops.nimg.cconv3(torch.zeros(1, 8, 8, 3), torch.zeros(5, 5, 3, 3), 1)        # no CPU kernel is registered
    # the dispatcher op itself is differentiable: same gradients as the Python front door above
    a2, w2 = a.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    torch.ops.nimg.conv2d(a2, w2, b.detach(), 1, 'leaky_relu').backward(gz)
    assert torch.equal(a2.grad, a.grad) and torch.equal(w2.grad, w.grad)
    # forward-only ops refuse inputs that require grad instead of silently cutting the graph; without grad they run
    img = g(natural_images(1, 16, 16, seed=9), dev)
    nf = g(rnd((5, 5, 3, 3), 8, -0.1, 0.1), dev)
    assert torch.ops.nimg.cconv3(img, nf, 1).shape == (1, 16, 16, 3)
    with pytest.raises(NotImplementedError):
        torch.ops.nimg.cconv3(img.clone().requires_grad_(True), nf, 1)


def test_torch_ops_autograd_matches_the_explicit_backward(dev):
    """torch.ops.nimg.* (neural-imaging_amd/torch_ops.py, round 5): a channel assembled from dispatcher ops alone -
    manipulations -> dJPEG -> constrained filter -> conv + LeakyReLU -> max-pool -> GAP / Dense / softmax / CE, plus the NIP
    loss - differentiated by torch.autograd on the GPU, against autograd of the float64 oracle on the CPU."""
    from neural_imaging_amd import ops, torch_ops  # noqa: F401  (importing torch_ops registers the ops)
    from oracle import nets as onets
    nimg = torch.ops.nimg
    n, h = 4, 32
    x0 = natural_images(n, h, h, seed=61)
    tgt = natural_images(n, h, h, seed=62)
    noise = rnd((n, h, h, 3), 63)
    kern = ot.fan_residual_init().astype(np.float32)
    w1, b1 = (0.1 * rnd((5, 5, 3, 8), 64)), 0.05 * rnd((8,), 65)
    wd, bd = 0.3 * rnd((8, 4), 66), 0.1 * rnd((4,), 67)
    labels = np.array([0, 1, 2, 3], np.int64)
    qt = ops.qtables_device(80, dev)

    def chain(P, lib):
        x = P['x']
        parts = [lib['sharpen'](x), lib['gaussian'](x), lib['resample'](x), lib['gamma'](x), lib['awgn'](x)]
        m = (parts[0] + parts[1] + parts[2] + parts[3] + parts[4]) / 5
        c = lib['djpeg'](m)
        r = lib['cconv'](c, P['kern'])
        a = lib['conv'](r, P['w1'], P['b1'])
        pl = lib['pool'](a)
        loss_ce = lib['head'](pl, P['wd'], P['bd'])
        return loss_ce + 0.01 * lib['mse'](m)

    mk = lambda a, d, t: torch.tensor(a, dtype=t, device=d, requires_grad=True)
    names = ('x', 'kern', 'w1', 'b1', 'wd', 'bd')
    vals = (x0, kern, w1, b1, wd, bd)
    Pg = {k: mk(v, dev, torch.float32) for k, v in zip(names, vals)}
    lab_g, tgt_g, noise_g = torch.tensor(labels, device=dev), g(tgt, dev), g(noise, dev)
    gpu = {'sharpen': lambda x: nimg.manipulation_sharpen(x, 1.0), 'gaussian': lambda x: nimg.manipulation_gaussian(x, 0.83),
           'resample': lambda x: nimg.manipulation_resample(x, 50.0), 'gamma': lambda x: nimg.manipulation_gamma(x, 3.0),
           'awgn': lambda x: nimg.manipulation_awgn(x, noise_g, 5.1 / 255), 'djpeg': lambda m: nimg.djpeg(m, qt, 'sin'),
           'cconv': lambda c, k: nimg.constrained_conv(c, k, 100.0), 'conv': lambda r, w, b: nimg.conv2d(r, w, b, 1, 'leaky_relu'),
           'pool': nimg.max_pool2, 'head': lambda a, w, b: nimg.fan_head(a, w, b, lab_g)[0], 'mse': lambda m: nimg.mse255(m, tgt_g)}
    loss_g = chain(Pg, gpu)
    grads_g = torch.autograd.grad(loss_g, [Pg[k] for k in names])

    Pc = {k: mk(v, 'cpu', torch.float64) for k, v in zip(names, vals)}
    mask = torch.tensor(ot.center_mask_2dfilter(5, 3), dtype=torch.float64)
    tgt_c, noise_c = to64(tgt), to64(noise)

    def head_c(a, w, b):
        probs = torch.softmax(a.mean(dim=(1, 2)) @ w + b, dim=1)
        return T.sparse_ce_from_probs(probs, labels)
    cpu = {'sharpen': lambda x: om.manipulation_sharpen(x, 1, hsv=True), 'gaussian': lambda x: om.manipulation_gaussian(x, 5, 0.83),
           'resample': lambda x: om.manipulation_resample(x, 50), 'gamma': lambda x: om.manipulation_gamma(x, 3.0),
           'awgn': lambda x: om.manipulation_awgn(x, 5.1 / 255, noise_c), 'djpeg': lambda m: odj.djpeg_torch(m, 80, 'sin')[0],
           'cconv': lambda c, k: T.constrained_conv(c, k, mask), 'conv': lambda r, w, b: T.leaky_relu(T.conv2d(r, w, b)),
           'pool': T.max_pool2, 'head': head_c, 'mse': lambda m: T.mse255(m, tgt_c)}
    loss_c = chain(Pc, cpu)
    grads_c = torch.autograd.grad(loss_c, [Pc[k] for k in names])
    assert abs(float(loss_g) - float(loss_c)) <= 1e-4 * max(1.0, abs(float(loss_c)))
    for k, a, b in zip(names, grads_g, grads_c):
        assert_close(a.cpu().numpy(), b.numpy(), 1e-7, 2e-3, what='torch.ops.nimg autograd: d loss / d ' + k)

    # the decoder tail of the UNet: Conv2DTranspose(2x2, stride 2) -> depth_to_space(2) + straight-through clip
    xt, wt, bt = rnd((2, 6, 6, 8), 70), 0.3 * rnd((2, 2, 12, 8), 71), 0.1 * rnd((12,), 72)
    tg = natural_images(2, 24, 24, seed=73)
    Qg = [mk(v, dev, torch.float32) for v in (xt, wt, bt)]
    lg = nimg.mse255(nimg.depth_to_space_clip(nimg.conv_transpose2x2(*Qg)), g(tg, dev))
    gg = torch.autograd.grad(lg, Qg)
    Qc = [mk(v, 'cpu', torch.float64) for v in (xt, wt, bt)]
    lc = T.mse255(T.clip_ste(T.depth_to_space(T.conv2d_transpose_2x2(*Qc), 2)), to64(tg))
    gc = torch.autograd.grad(lc, Qc)
    assert abs(float(lg) - float(lc)) <= 1e-5 * float(lc)
    for a, b, k in zip(gg, gc, ('x', 'kernel', 'bias')):
        assert_close(a.cpu().numpy(), b.numpy(), 1e-7, 2e-4, what='conv_transpose2x2 -> depth_to_space_clip: d loss / d ' + k)
    # inference mode reaches the kernels through the backend key
    with torch.inference_mode():
        assert nimg.max_pool2(g(rnd((1, 8, 8, 8), 74), dev)).shape == (1, 4, 4, 8)


@pytest.mark.parametrize('n,h', [(3, 128), (2, 20), (5, 64)])
def test_row_streaming_convolution_equals_the_tile_kernels(dev, n, h, monkeypatch):
    """csrc/conv3_rows.hip (the UNet's level-1 layers in throughput mode: 3x3, 32 output channels, 128-pixel rows, bf16 storage):
    forward with and without the pooled tensor, two-tensor and 64-channel inputs, the input-gradient form with the previous
    layer's LeakyReLU' - the same bits as the tile kernels (same products, same summation order), whatever the band split."""
    from neural_imaging_amd import ops
    wd = 128
    bf = lambda a: g(a, dev).to(torch.bfloat16)
    same = lambda a, b: torch.equal(a.view(torch.int16), b.view(torch.int16))
    try:
        ops.set_compute('bf16')
        for c1, c2 in ((32, 0), (32, 32), (64, 0)):
            x = bf(rnd((n, h, wd, c1), 80 + c1))
            x2 = bf(rnd((n, h, wd, c2), 81)) if c2 else None
            w, b = g(0.1 * rnd((3, 3, c1 + c2, 32), 82), dev), g(0.1 * rnd((32,), 83), dev)
            for act in ('leaky_relu', None):
                monkeypatch.setattr(ops, 'ROWS_CONV', False)
                ref = ops.conv2d(x, w, b, x2=x2, act=act, out_bf16=True)
                monkeypatch.setattr(ops, 'ROWS_CONV', True)
                assert ops.rows_conv_ok(x, x2, 3, 1, 32, (h, wd), (1, 1), 0, ref, None, None, act)
                assert same(ops.conv2d(x, w, b, x2=x2, act=act, out_bf16=True), ref), (c1, c2, act)
        x = bf(rnd((n, h, wd, 32), 84))
        w, b = g(0.1 * rnd((3, 3, 32, 32), 85), dev), g(0.1 * rnd((32,), 86), dev)
        monkeypatch.setattr(ops, 'ROWS_CONV', False)
        ra, rp = ops.conv2d_and_pool(x, w, b)
        dz, prev = bf(rnd((n, h, wd, 32), 87)), bf(rnd((n, h, wd, 32), 88))
        rd = ops.conv2d_dgrad(dz, w, (h, wd), act_mask=prev, out_bf16=True)
        monkeypatch.setattr(ops, 'ROWS_CONV', True)
        ga, gp = ops.conv2d_and_pool(x, w, b)
        assert same(ga, ra) and same(gp, rp)
        assert same(ops.conv2d_dgrad(dz, w, (h, wd), act_mask=prev, out_bf16=True), rd)
        # float32 result (ec12's input gradient) and a 64-channel gradient that leaves as two tensors (dc41's [up, skip])
        w64 = g(0.1 * rnd((3, 3, 64, 32), 92), dev)

        def grads(on):
            monkeypatch.setattr(ops, 'ROWS_CONV', on)
            o1 = torch.empty((n, h, wd, 32), dtype=torch.bfloat16, device=dev)
            o2 = torch.empty_like(o1)
            ops.conv2d_dgrad(dz, w64, (h, wd), out=o1, out2=o2)
            return ops.conv2d_dgrad(dz, w, (h, wd), act_mask=prev, out_bf16=False), o1, o2
        (f0, a0, b0), (f1, a1, b1) = grads(False), grads(True)
        assert f1.dtype == torch.float32 and torch.equal(f0, f1) and same(a0, a1) and same(b0, b1)
        # the UNet's first layer: 4 float32 RAW planes -> 32 channels
        x4, w4 = g(rnd((n, h, wd, 4), 93, 0, 1), dev), g(0.2 * rnd((3, 3, 4, 32), 94), dev)
        for act in ('leaky_relu', None):
            monkeypatch.setattr(ops, 'ROWS_CONV', False)
            ref4 = ops.conv2d(x4, w4, b, act=act, out_bf16=True)
            monkeypatch.setattr(ops, 'ROWS_CONV', True)
            assert same(ops.conv2d(x4, w4, b, act=act, out_bf16=True), ref4), act
        # the UNet's last layer: 32 -> 12 channels written as the clipped depth_to_space image
        w12, b12 = g(0.3 * rnd((3, 3, 32, 12), 90), dev), g(0.2 * rnd((12,), 91), dev)
        want = ops.d2s_clip(ops.conv2d(x, w12, b12), 1.0, 0.0, True)
        assert ops.rows_d2s_ok(x, w12)
        got = ops.conv3_rows_d2s(x, w12, b12)
        assert torch.equal(got, want) and float(got.min()) == 0.0 and float(got.max()) == 1.0
        # second level of the UNet (opt-in form): 64-pixel rows, 32 | 64 -> 64 channels, forward and the input-gradient form with a mask
        monkeypatch.setattr(ops, 'ROWS_LEVEL2', True)
        h2 = 64 if h >= 64 else (h // 4) * 4
        for c1 in (32, 64):
            x2l = bf(rnd((n, h2, 64, c1), 95 + c1))
            wl, bl = g(0.1 * rnd((3, 3, c1, 64), 96), dev), g(0.1 * rnd((64,), 97), dev)
            prevl = bf(rnd((n, h2, 64, 64), 98))
            wg = g(0.1 * rnd((3, 3, 64, c1), 99), dev)             # a layer c1... whose gradient w.r.t. its 64-channel input is taken
            res = {}
            for on in (False, True):
                monkeypatch.setattr(ops, 'ROWS_CONV', on)
                res[on] = (ops.conv2d(x2l, wl, bl, act='leaky_relu', out_bf16=True),
                           ops.conv2d_dgrad(x2l, wg, (h2, 64), act_mask=prevl, out_bf16=True) if c1 == 64 else None)
            assert ops.rows_conv_ok(x2l, None, 3, 1, 64, (h2, 64), (1, 1), 0, res[True][0], None, None, 'leaky_relu')
            assert same(res[False][0], res[True][0]), c1
            if c1 == 64:
                assert same(res[False][1], res[True][1])
        # shapes the streaming form does not take fall through to the tile kernels
        assert not ops.rows_conv_ok(bf(rnd((1, 16, 32, 32), 89)), None, 3, 1, 32, (16, 32), (1, 1), 0, ref, None, None, None)
    finally:
        ops.set_compute('f32')
