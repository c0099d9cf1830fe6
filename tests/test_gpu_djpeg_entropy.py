"""The dJPEG rate term on the device (csrc/djpeg_entropy.hip) against the float64 restatement of
tests/djpeg_entropy_ref.py: value, gradients to the image and to the tables, the semantics of the C ABI, guard bytes, error codes,
and the model / workflow / dispatcher layers above it.  Cases, tolerances and their measured floors: djpeg_entropy_ref.CASES."""
import numpy as np
import pytest
import torch

import djpeg_entropy_ref as R
from util import natural_images

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    return torch.device('cuda', 0)


def g(a, dev):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(dev).contiguous()


def same(a, b):
    """Two runs of the forward pass: equal to float32 rounding (the float64 LDS atomics of a workgroup arrive in any order)."""
    return abs(float(a) - float(b)) <= 1e-6 * abs(float(b))


class Guarded(object):
    """`nbytes` of device memory between two runs of 0xa5 bytes."""

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


def run_case(dev, name, mode, coef=1.0):
    """Forward and backward (with the table gradient) inside guard bytes: (H, gx, dq (2,8,8)) as float64 numpy."""
    from neural_imaging_amd import _lib, ops
    x, q = R.case_inputs(name)
    n, h, w, _ = x.shape
    xd, qd = g(x, dev), g(q, dev)
    ws = Guarded(_lib.load().nimg_djpeg_entropy_workspace_bytes(n, h, w), dev)
    ent, gx, dq = Guarded(4, dev), Guarded(x.size * 4, dev), Guarded(128 * 4, dev)
    ops.djpeg_entropy_fwd(xd, qd, mode, ws=ws.bytes, out=ent.f32(1))
    ops.djpeg_entropy_bwd(xd, qd, ws.bytes, coef, mode, out=gx.f32(*x.shape), dq=dq.f32(2, 8, 8))
    torch.cuda.synchronize(dev)
    for what, b in (('entropy', ent), ('gx', gx), ('dq', dq), ('workspace', ws)):
        assert b.intact(), '{}: guard bytes overwritten'.format(what)
    return (float(ent.f32(1)[0]), gx.f32(*x.shape).cpu().numpy().astype(np.float64),
            dq.f32(2, 8, 8).cpu().numpy().astype(np.float64))


def assert_grad(got, ref, tol, what):
    assert np.isfinite(got).all(), what
    diff, bound = np.abs(got - ref), R.GRAD_ATOL + tol * np.abs(ref).max()
    print('{}: max|diff| {:.3e}, max|ref| {:.3e}, bound {:.3e}'.format(what, diff.max(), np.abs(ref).max(), bound))
    assert diff.max() <= bound, '{}: max|diff| {:.3e} > {:.3e} (max|ref| {:.3e})'.format(what, diff.max(), bound, np.abs(ref).max())


@pytest.mark.parametrize('mode', R.MODES)
@pytest.mark.parametrize('name', list(R.CASES))
def test_value_and_gradients(dev, name, mode):
    from neural_imaging_amd import ops
    H, gx, dq = run_case(dev, name, mode)
    H_ref, gx_ref, dq_ref = R.reference(name, mode)
    if mode == 'soft':
        # the bit-exact witness: H is the entropy of the index tensor nimg_djpeg_fwd writes
        x, q = R.case_inputs(name)
        idx = ops.djpeg_fwd(g(x, dev), g(q, dev), 'soft', want_mask=False, want_idx=True)[2]
        H_idx = float(R.entropy_of(idx.cpu().to(torch.float64)))
        print('{} soft: H {:.7f}, entropy(idx) {:.7f}, float64 reference {:.7f}'.format(name, H, H_idx, H_ref))
        assert abs(H - H_idx) <= R.VALUE_TOL, (H, H_idx)
    else:
        print('{} {}: H {:.7f}, float64 reference {:.7f}'.format(name, mode, H, H_ref))
        assert abs(H - H_ref) <= R.VALUE_TOL, (H, H_ref)
    tol = R.CASES[name]['grad_tol']
    assert_grad(gx, gx_ref, tol, '{} {} gx'.format(name, mode))
    assert_grad(dq, dq_ref, tol, '{} {} dq'.format(name, mode))
    if mode == 'soft' and R.CASES[name]['q'] in ('q60', 'nonint'):
        # every value in range and at an integer: the estimator's derivative vanishes there
        assert np.abs(gx_ref).max() < 1e-20 and np.abs(gx).max() < 1e-9 and np.abs(dq).max() < 1e-9


@pytest.mark.parametrize('name,mode', [('q60', 'sin'), ('non-integer-tables', 'harmonic'), ('ragged-strip-q60', 'sin')])
def test_abi_semantics(dev, name, mode):
    from neural_imaging_amd import ops
    x, q = R.case_inputs(name)
    xd, qd = g(x, dev), g(q, dev)
    ent, ws = ops.djpeg_entropy_fwd(xd, qd, mode)
    dq1 = torch.zeros(2, 8, 8, device=dev)
    gx1 = ops.djpeg_entropy_bwd(xd, qd, ws, 1.0, mode, dq=dq1)
    sx, sq = float(gx1.abs().max()), float(dq1.abs().max())
    assert sx > 0 and sq > 0
    # coef is linear
    dq2 = torch.zeros(2, 8, 8, device=dev)
    gx2 = ops.djpeg_entropy_bwd(xd, qd, ws, 2.5, mode, dq=dq2)
    assert float((gx2 - 2.5 * gx1).abs().max()) <= 1e-6 * 2.5 * sx and float((dq2 - 2.5 * dq1).abs().max()) <= 1e-6 * 2.5 * sq
    # accumulate adds onto what is there, for the image and for the tables independently
    rng = np.random.default_rng(7)
    gx0, dq0 = g(rng.normal(0, sx, x.shape), dev), g(rng.normal(0, sq, (2, 8, 8)), dev)
    gxa, dqa = gx0.clone(), dq0.clone()
    assert ops.djpeg_entropy_bwd(xd, qd, ws, 1.0, mode, out=gxa, accumulate=True, dq=dqa, accumulate_dq=True) is gxa
    assert float((gxa - (gx0 + gx1)).abs().max()) <= 1e-6 * float((gx0.abs() + gx1.abs()).max())
    assert float((dqa - (dq0 + dq1)).abs().max()) <= 1e-6 * float((dq0.abs() + dq1.abs()).max())
    gxb, dqb = gx0.clone(), dq0.clone()
    ops.djpeg_entropy_bwd(xd, qd, ws, 1.0, mode, out=gxb, accumulate=False, dq=dqb, accumulate_dq=True)
    assert float((gxb - gx1).abs().max()) <= 1e-6 * sx and float((dqb - (dq0 + dq1)).abs().max()) <= 1e-6 * float((dq0.abs() + dq1.abs()).max())
    # dq=None leaves the tables alone and gives the same image gradient (integer tables: the fast division is the exact one)
    gxn = ops.djpeg_entropy_bwd(xd, qd, ws, 1.0, mode)
    assert float((gxn - gx1).abs().max()) <= 1e-6 * sx
    with pytest.raises(ValueError):
        ops.djpeg_entropy_bwd(xd, qd, ws, 1.0, mode, accumulate=True)
    # forward twice, then backward == forward once, then backward - also after the backward passes above re-used the partial-sum
    # region of the workspace.  To float32 rounding, not bit for bit: a workgroup's float64 LDS atomics arrive in any order.
    ent2, _ = ops.djpeg_entropy_fwd(xd, qd, mode, ws=ws)
    ops.djpeg_entropy_fwd(xd, qd, mode, ws=ws)
    dq3 = torch.zeros(2, 8, 8, device=dev)
    gx3 = ops.djpeg_entropy_bwd(xd, qd, ws, 1.0, mode, dq=dq3)
    assert same(ent2[0], ent[0])
    assert float((gx3 - gx1).abs().max()) <= 1e-6 * sx and float((dq3 - dq1).abs().max()) <= 1e-6 * sq


def test_error_codes_on_the_device(dev):
    from neural_imaging_amd import ops
    x, q = R.case_inputs('q60')
    xd, qd = g(x, dev), g(q, dev)
    ent, ws = ops.djpeg_entropy_fwd(xd, qd, 'sin')
    short = ws[:ws.numel() - 16]
    with pytest.raises(RuntimeError, match='NIMG_ERR_WORKSPACE'):
        ops.djpeg_entropy_fwd(xd, qd, 'sin', ws=short)
    with pytest.raises(RuntimeError, match='NIMG_ERR_WORKSPACE'):
        ops.djpeg_entropy_bwd(xd, qd, short, 1.0, 'sin')
    with pytest.raises(RuntimeError, match='NIMG_ERR_ARG'):
        ops.djpeg_entropy_fwd(torch.zeros(1, 12, 8, 3, device=dev), qd, 'sin', ws=ws)
    with pytest.raises(RuntimeError, match='NIMG_ERR_ARG'):
        ops.djpeg_entropy_bwd(torch.zeros(1, 8, 20, 3, device=dev), qd, ws, 1.0, 'sin')
    with pytest.raises(KeyError):
        ops.djpeg_entropy_fwd(xd, qd, 'bogus', ws=ws)
    with pytest.raises(ValueError):
        ops.djpeg_entropy_fwd(torch.zeros(1, 8, 8, 4, device=dev), qd, 'sin')
    # an empty batch is a no-op
    e0, _ = ops.djpeg_entropy_fwd(torch.zeros(0, 8, 8, 3, device=dev), qd, 'sin', out=torch.full((1,), 7.0, device=dev))
    assert float(e0[0]) == 7.0
    # the refusals left the good workspace good
    assert same(ops.djpeg_entropy_fwd(xd, qd, 'sin', ws=ws)[0][0], ent[0])


def test_dispatcher_op_under_autograd(dev):
    import neural_imaging_amd.torch_ops  # noqa: F401  (registers torch.ops.nimg)
    from neural_imaging_amd import ops
    x, q = R.case_inputs('q60')
    xd, qd = g(x, dev).requires_grad_(True), g(q, dev)
    H = torch.ops.nimg.djpeg_entropy(xd, qd, 'sin')
    assert H.dim() == 0 and H.requires_grad
    (3.0 * H).backward()
    ent, ws = ops.djpeg_entropy_fwd(xd.detach(), qd, 'sin')
    gx = ops.djpeg_entropy_bwd(xd.detach(), qd, ws, 1.0, 'sin')
    assert same(H, ent[0])
    assert float((xd.grad - 3.0 * gx).abs().max()) <= 1e-6 * 3.0 * float(gx.abs().max())
    with torch.no_grad():
        assert same(torch.ops.nimg.djpeg_entropy(xd, qd, 'sin'), ent[0])


class _Validation(object):
    def __init__(self, x):
        self.x, self.count_validation = x, x.shape[0]

    def next_validation_batch(self, b, batch_size):
        return self.x[b * batch_size:(b + 1) * batch_size]


def test_model_reports_and_differentiates_the_rate(dev):
    from neural_imaging_amd import ops
    from neural_imaging_amd.models import jpeg
    from neural_imaging_amd.training.validation import validate_jpeg
    x, _ = R.case_inputs('q60')
    tables = R.noninteger_tables()
    m = jpeg.JPEG(60, 'sin', trainable=True, device=dev, entropy_weight=0.3)
    m.load_state_dict({'Q_mtx_luma': tables[0], 'Q_mtx_chroma': tables[1]})
    xd, qd = g(x, dev), g(tables, dev)
    ent, ws = ops.djpeg_entropy_fwd(xd, qd, 'sin')
    y, H = m.process(x, return_entropy=True)
    assert isinstance(H, float) and same(H, ent[0])
    assert torch.equal(y.t, ops.djpeg_fwd(xd, qd, 'sin', want_mask=False)[0])
    assert not isinstance(m.process(x), tuple)
    # an explicit other quality: the entropy at that quality's IJG tables
    assert same(m.process(x, quality=95, return_entropy=True)[1], ops.djpeg_entropy_fwd(xd, g(R.ijg(95), dev), 'sin')[0][0])
    # forward / backward: the ctx carries the entropy; entropy_coef adds to the image gradient and to the table gradients
    dy = g(np.random.default_rng(3).normal(0, 1e-3, x.shape), dev)
    _, ctx = m.forward(xd, training=True)
    assert ctx['entropy'].shape == (1,) and same(ctx['entropy'][0], ent[0])
    gx_d = m.backward(ctx, dy).clone()
    dq_d = m._model.flat_grad.clone()
    gx_both = m.backward(ctx, dy, entropy_coef=0.7)
    dq_both = m._model.flat_grad.clone()
    dq_h = torch.zeros(128, device=dev)
    gx_h = ops.djpeg_entropy_bwd(xd, qd, ws, 0.7, 'sin', dq=dq_h)
    assert float(gx_h.abs().max()) > 0 and float(dq_h.abs().max()) > 0
    assert float((gx_both - (gx_d + gx_h)).abs().max()) <= 1e-6 * float((gx_d.abs() + gx_h.abs()).max())
    assert float((dq_both - (dq_d + dq_h)).abs().max()) <= 1e-6 * float((dq_d.abs() + dq_h.abs()).max())
    # validate_jpeg reports it; the default model reports NaN, as before
    rec = validate_jpeg(m, _Validation(x), batch_size=x.shape[0])
    assert same(rec['entropy'], H) and np.isfinite(rec['psnr'])
    plain = jpeg.JPEG(60, 'sin', device=dev)
    assert np.isnan(plain.process(x, return_entropy=True)[1]) and np.isnan(validate_jpeg(plain, _Validation(x))['entropy'])
    with pytest.raises(ValueError):
        plain.backward(plain.forward(xd, training=True)[1], dy, entropy_coef=1.0)


def test_workflow_trains_with_the_rate_term(dev):
    from neural_imaging_amd import ops
    from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification
    from util import bayer_from_rgb
    w, lam = 0.3, 0.5
    tables = R.noninteger_tables()

    def workflow(weight):
        params = {'quality': 60, 'codec': 'sin', 'trainable': True}
        if weight is not None:
            params['entropy_weight'] = weight
        dist = {'downsampling': 'none', 'compression': 'jpeg', 'compression_params': params}
        wf = ManipulationClassification('INet', manipulations=['sharpen:1', 'gaussian:1'], distribution=dist,
                                        trainable={'nip', 'dcn'}, raw_patch_size=32, device=dev)
        wf.codec.load_state_dict({'Q_mtx_luma': tables[0], 'Q_mtx_chroma': tables[1]})
        return wf

    rate, plain = workflow(w), workflow(None)
    plain.nip.load_state_dict(rate.nip.state_dict())
    plain.fan.load_state_dict(rate.fan.state_dict())
    assert ' H+0.3' in rate.summary() and 'H+' not in plain.summary()
    rgb = natural_images(2, 64, 64, seed=3)
    raw = bayer_from_rgb(rgb)
    # the reported entropy is the op's, on the codec's input
    _, c, C, ent, _ = rate.run_workflow(raw)
    cd, qd = torch.as_tensor(c.numpy()).to(dev), g(tables, dev)
    H, ws = ops.djpeg_entropy_fwd(cd, qd, 'sin')
    assert same(ent, H[0]) and np.isfinite(float(ent))
    assert same(rate.run_compression(c, return_entropy=True)[1], H[0])
    assert np.isnan(plain.run_workflow(raw)[3]) and np.isnan(plain.run_compression(c, return_entropy=True)[1])
    dq_h = torch.zeros(128, device=dev)
    ops.djpeg_entropy_bwd(cd, qd, ws, lam * w, 'sin', dq=dq_h)
    # one step of each: the codec term and the table gradients differ by exactly the rate term
    loss_r, parts_r = rate.training_step(raw, rgb, lambda_nip=0.1, lambda_dcn=lam, learning_rate=1e-4)
    loss_p, parts_p = plain.training_step(raw, rgb, lambda_nip=0.1, lambda_dcn=lam, learning_rate=1e-4)
    rate.finish_pending()
    plain.finish_pending()
    assert np.isfinite(float(loss_r)) and np.isfinite(float(parts_r['dcn']))
    mse_term = float(parts_p['dcn'])                       # MSE(c, C) on [0,1] images = mse255 / 255^2
    assert abs(float(parts_r['dcn']) - (mse_term + w * float(H[0]))) <= 1e-6 * (mse_term + w * float(H[0]))
    assert abs(float(loss_r) - (float(loss_p) + lam * w * float(H[0]))) <= 1e-5 * abs(float(loss_r))
    g_r, g_p = rate.codec._model.flat_grad, plain.codec._model.flat_grad
    assert float(dq_h.abs().max()) > 0
    assert float((g_r - (g_p + dq_h)).abs().max()) <= 1e-5 * float((g_p.abs() + dq_h.abs()).max())
    # and the tables moved
    assert float((rate.codec._codec_model.params.flat - g(tables[:2], dev).reshape(-1)).abs().max()) > 0
