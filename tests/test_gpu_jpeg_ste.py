"""
The real JPEG codec as a training forward on the GPU (csrc/jpeg_ste.hip): nimg_jpeg_ste_fwd against its numpy
restatement (tests/jpeg_ste_ref.py) and against the device codec it must equal, bit for bit - the arithmetic is integer, there is no
tolerance anywhere - then the C ABI, the model codecs 'libjpeg+identity' / '+sin' / '+harmonic', the dispatcher op and the workflow.
"""
import numpy as np
import pytest
import torch

import djpeg_cases as C
import jpeg_ste_ref as S
from util import bayer_from_rgb, natural_images

pytestmark = pytest.mark.gpu

SUBS = ['4:4:4', '4:2:2', '4:2:0']
FACTORS = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}
ROUNDINGS = ['identity', 'sin', 'harmonic']


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda', 0)


def g(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)          # a copy: the references are read-only


def device_tables(q, dev):
    """(3, 64) int64 tables -> the (1, 3, 64) int16 device tensor holding the uint16 entries."""
    return g(np.asarray(q).astype(np.uint16).view(np.int16).reshape(1, 3, 64), dev)


def codec_image(x, sub, q):
    """What the device codec decodes from the file it writes for x: at a quality, or with the caller's tables."""
    from neural_imaging_amd.compression.jpeg_helpers import device_codec
    if q == 'three':
        return device_codec(x, None, sub, want_bytes=False, qtables=S.tables_of(q).astype(np.uint16))[0]
    return device_codec(x, q, sub, want_bytes=False)[0]


# ---- 1. forward, exact -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.CASES, ids=S.CASE_IDS)
def test_forward_is_the_restatement_and_the_device_codec(dev, case):
    from neural_imaging_amd import ops
    sub, shape, kind, q = case
    ref = S.reference(*case)
    x = g(S.image(shape, kind), dev)
    y, mask, err = ops.jpeg_ste_fwd(x, device_tables(S.tables_of(q), dev), *FACTORS[sub])
    assert y.dtype == torch.float32 and mask.dtype == torch.uint8 and tuple(mask.shape) == shape
    assert torch.equal(y, g(ref['y'], dev))
    assert torch.equal(y, codec_image(x, sub, q))
    assert np.array_equal(mask.cpu().numpy(), ref['mask'])
    assert int(err.item()) == 0


# ---- 2. without a mask, in place ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub, shape', S.SHAPES, ids=S.SHAPE_IDS)
def test_without_a_mask_and_in_place(dev, sub, shape):
    from neural_imaging_amd import ops
    x = g(S.image(shape, 'saturated'), dev)
    qt = device_tables(S.tables_of(50), dev)
    y, mask, _ = ops.jpeg_ste_fwd(x, qt, *FACTORS[sub])
    out = torch.full_like(x, -1.0)
    y2, none, _ = ops.jpeg_ste_fwd(x, qt[0], *FACTORS[sub], want_mask=False, out=out)          # (3, 64) tables serve as (1, 3, 64)
    assert none is None and y2 is out and torch.equal(out, y)


# ---- 3. one user-sized shape per sub-sampling ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub', SUBS)
def test_user_sized_batch_equals_the_device_codec(dev, sub):
    from neural_imaging_amd import ops
    x = g(natural_images(*S.USER_SHAPE, seed=75), dev)
    y, mask, err = ops.jpeg_ste_fwd(x, device_tables(S.tables_of(75), dev), *FACTORS[sub])
    assert torch.equal(y, codec_image(x, sub, 75)) and int(err.item()) == 0
    share = S.clear_share(mask.cpu().numpy())
    assert 0.0 <= share < 0.5                                           # natural images clip little; all bits above 2 stay clear
    assert not bool((mask >> 3).any())


# ---- 4. conversion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub, shape', S.SHAPES, ids=S.SHAPE_IDS)
def test_values_outside_the_unit_interval_clamp_per_value(dev, sub, shape):
    from neural_imaging_amd import ops
    ref = S.reference_unclipped(sub, shape, 50)
    x = g(S.image(shape, 'unclipped'), dev)
    assert float(x.min()) < 0 and float(x.max()) > 1
    y, mask, _ = ops.jpeg_ste_fwd(x, device_tables(S.tables_of(50), dev), *FACTORS[sub])
    assert torch.equal(y, g(ref['y'], dev)) and np.array_equal(mask.cpu().numpy(), ref['mask'])


# ---- 5. ABI ----------------------------------------------------------------------------------------------------------------------------
GUARD = 256


class Guarded(object):
    """A device buffer of `nbytes` with GUARD poisoned bytes in front and behind."""

    def __init__(self, nbytes, dev, poison=0xA5):
        self.n, self.poison = int(nbytes), poison
        self.buf = torch.full((self.n + 2 * GUARD,), poison, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == self.poison).all()) and bool((self.buf[GUARD + self.n:] == self.poison).all())

    def untouched(self):
        return bool((self.buf == self.poison).all())


def raw_call(lib, x, qt, shape, hs, vs, y, mask, err, ws, ws_bytes):
    n, h, w = shape
    return lib.nimg_jpeg_ste_fwd(x, qt, n, h, w, hs, vs, y, mask, err, ws, ws_bytes, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('sub, shape', [('4:4:4', (3, 8, 136)), ('4:2:2', (2, 24, 80)), ('4:2:0', (2, 48, 80))])
def test_abi_stays_inside_its_buffers(dev, sub, shape):
    from neural_imaging_amd import _lib
    lib = _lib.load()
    hs, vs = FACTORS[sub]
    n, h, w = shape
    ref = S.reference(sub, shape, 'saturated', 50)
    x = g(S.image(shape, 'saturated'), dev)
    qt = device_tables(S.tables_of(50), dev)
    need = lib.nimg_jpeg_ste_workspace_bytes(n, h, w, hs, vs)
    assert need == (0 if hs == 1 else 2 * n * h * w // (hs * vs))
    y, mask, ws = Guarded(n * h * w * 12, dev), Guarded(n * h * w, dev), Guarded(need, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    assert raw_call(lib, x.data_ptr(), qt.data_ptr(), shape, hs, vs, y.ptr, mask.ptr, err.data_ptr(), ws.ptr, need) == 0
    torch.cuda.synchronize(dev)
    assert y.guards_intact() and mask.guards_intact() and ws.guards_intact()
    assert torch.equal(y.body().view(torch.float32).view(n, h, w, 3), g(ref['y'], dev))
    assert np.array_equal(mask.body().view(n, h, w).cpu().numpy(), ref['mask'])
    assert int(err.item()) == 0
    # a table entry of 0 or of 300 is clamped, reported, and nothing leaves the buffers
    for bad in (0, 300):
        t = S.tables_of(50).copy()
        t[1, 7] = bad
        y2, mask2, ws2 = Guarded(n * h * w * 12, dev), Guarded(n * h * w, dev), Guarded(need, dev)
        err.zero_()
        assert raw_call(lib, x.data_ptr(), device_tables(t, dev).data_ptr(), shape, hs, vs, y2.ptr, mask2.ptr, err.data_ptr(), ws2.ptr,
                        need) == 0
        torch.cuda.synchronize(dev)
        assert int(err.item()) == 1
        assert y2.guards_intact() and mask2.guards_intact() and ws2.guards_intact()
        t[1, 7] = min(max(bad, 1), 255)
        want = S.restate(S.ref.to_bytes(S.image(shape, 'saturated')), t, sub)
        assert torch.equal(y2.body().view(torch.float32).view(n, h, w, 3), g(want['y'], dev))


def test_abi_refusals_leave_the_output_untouched(dev):
    from neural_imaging_amd import _lib
    lib = _lib.load()
    ARG, WORKSPACE = -1, -3
    shape = (2, 48, 80)
    n, h, w = shape
    x = g(S.image(shape, 'saturated'), dev)
    qt = device_tables(S.tables_of(50), dev)
    need = lib.nimg_jpeg_ste_workspace_bytes(n, h, w, 2, 2)
    y, mask, ws = Guarded(n * h * w * 12, dev), Guarded(n * h * w, dev), Guarded(need, dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    a = dict(x=x.data_ptr(), qt=qt.data_ptr(), shape=shape, hs=2, vs=2, y=y.ptr, mask=mask.ptr, err=err.data_ptr(), ws=ws.ptr,
             ws_bytes=need)
    assert raw_call(lib, **dict(a, ws_bytes=need - 1)) == WORKSPACE
    assert raw_call(lib, **dict(a, shape=(2, 40, 80))) == ARG            # ragged: h % 16
    assert raw_call(lib, **dict(a, shape=(2, 48, 72))) == ARG            # ragged: w % 16
    assert raw_call(lib, **dict(a, hs=1, vs=2)) == ARG
    assert raw_call(lib, **dict(a, hs=2, vs=1, shape=(2, 48, 72))) == ARG
    assert raw_call(lib, **dict(a, shape=(2, 4104, 80))) == ARG          # beyond nimg_jpeg_transform's limits
    for name in ('x', 'qt', 'y', 'err'):
        assert raw_call(lib, **dict(a, **{name: None})) == ARG
    assert raw_call(lib, **dict(a, shape=(0, 48, 80))) == 0              # an empty batch: OK, nothing launched
    assert raw_call(lib, None, None, (0, 48, 80), 2, 2, None, None, None, None, 0) == 0
    torch.cuda.synchronize(dev)
    assert y.untouched() and mask.untouched() and ws.untouched() and int(err.item()) == 0
    assert lib.nimg_jpeg_ste_workspace_bytes(0, 48, 80, 2, 2) == 0 and lib.nimg_jpeg_ste_workspace_bytes(2, 40, 80, 2, 2) == 0
    assert raw_call(lib, **dict(a, mask=None)) == 0                      # the mask alone may be null


def test_ops_refusals(dev):
    from neural_imaging_amd import ops
    x = g(S.image((2, 48, 80), 'saturated'), dev)
    qt = device_tables(S.tables_of(50), dev)
    with pytest.raises(RuntimeError, match='workspace|WORKSPACE'):
        ops.jpeg_ste_fwd(x, qt, 2, 2, workspace=torch.empty(10, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError):
        ops.jpeg_ste_fwd(x, qt.repeat(2, 1, 1), 2, 2)                    # one table set for the batch
    with pytest.raises(RuntimeError):
        ops.jpeg_ste_fwd(x, qt.float(), 2, 2)
    y, mask, _ = ops.jpeg_ste_fwd(x[:0], qt, 2, 2)
    assert tuple(y.shape) == (0, 48, 80, 3) and tuple(mask.shape) == (0, 48, 80)


# ---- 6. model: equality with the real codec -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub', SUBS)
def test_model_forward_equals_the_libjpeg_codec(dev, sub):
    from neural_imaging_amd.models.jpeg import JPEG
    x = natural_images(2, 48, 80, seed=81)
    a = JPEG(75, 'libjpeg+identity', subsampling=sub, device=dev).process(x).numpy()
    b = JPEG(75, 'libjpeg', subsampling=sub, device=dev).process(x).numpy()
    assert np.array_equal(a, b)
    m = JPEG(75, 'libjpeg+sin', subsampling=sub, device=dev)
    assert np.array_equal(m.process(x, quality=40).numpy(), JPEG(40, 'libjpeg', subsampling=sub, device=dev).process(x).numpy())
    y, sizes = m.process_files(x)                                        # the helpers work: the files hold the same image
    assert np.array_equal(y.cpu().numpy() if hasattr(y, 'cpu') else np.asarray(y), b) and len(sizes) == 2


# ---- 7. model: backward through the existing ops ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('rounding', ROUNDINGS)
def test_model_backward_is_the_differentiable_adjoint(dev, sub, rounding):
    from neural_imaging_amd import ops
    from neural_imaging_amd.models.jpeg import JPEG
    shape = (2, 48, 80)
    x = g(S.image(shape, 'saturated'), dev)
    gy = g(C.gradient(shape), dev)
    m = JPEG(50, 'libjpeg+' + rounding, subsampling=sub, device=dev)
    y0, none = m.forward(x)
    assert none is None
    y, ctx = m.forward(x, training=True)
    assert sorted(ctx) == ['learned', 'mask', 'q', 'x'] and ctx['learned'] is False and ctx['x'] is x
    ref = S.reference(sub, shape, 'saturated', 50)
    assert torch.equal(y, y0) and torch.equal(y, g(ref['y'], dev)) and np.array_equal(ctx['mask'].cpu().numpy(), ref['mask'])
    q = g(S.tables_of(50).astype(np.float32).reshape(3, 8, 8), dev)       # libjpeg's integer tables, as floats
    assert ctx['q'].dtype == torch.float32 and torch.equal(ctx['q'], q)
    gx = m.backward(ctx, gy)
    hs, vs = FACTORS[sub]
    want = ops.djpeg_bwd(x, gy, ctx['mask'], q, rounding) if sub == '4:4:4' else ops.djpeg_sub_bwd(x, gy, ctx['mask'], q, rounding, hs, vs)
    assert torch.equal(gx, want)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().max()) > 0
    with pytest.raises(ValueError):
        m.backward(ctx, gy, entropy_coef=0.5)                            # no rate term on a real codec


# ---- 8. learned tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub', ['4:4:4', '4:2:0'])
def test_learned_tables(dev, sub):
    from neural_imaging_amd import ops
    from neural_imaging_amd.models.jpeg import JPEG
    shape = (2, 48, 80)
    x = g(S.image(shape, 'saturated'), dev)
    gy = g(C.gradient(shape), dev)
    m = JPEG(60, 'libjpeg+sin', trainable=True, subsampling=sub, device=dev)
    d = JPEG(60, 'sin', trainable=True, subsampling=sub, device=dev)
    ql, qc = C.frac_pair()                                                 # trained-looking weights: not integers
    for model in (m, d):
        model._model.p['Q_mtx_luma'].copy_(g(ql, dev))
        model._model.p['Q_mtx_chroma'].copy_(g(qc, dev))
    y, ctx = m.forward(x, training=True)
    files, _ = d.process_files(x.cpu().numpy())
    assert np.array_equal(y.cpu().numpy(), files.cpu().numpy() if hasattr(files, 'cpu') else np.asarray(files))
    assert np.array_equal(m.file_tables()[0], d.file_tables()[0])
    assert ctx['learned'] is True and torch.equal(ctx['q'], g(np.stack([ql, qc, qc]), dev))
    m._model.flat_grad.zero_()
    gx = m.backward(ctx, gy)
    dq = torch.zeros(128, device=dev)
    hs, vs = FACTORS[sub]
    want = ops.djpeg_bwd(x, gy, ctx['mask'], ctx['q'], 'sin', dq=dq) if sub == '4:4:4' else \
        ops.djpeg_sub_bwd(x, gy, ctx['mask'], ctx['q'], 'sin', hs, vs, dq=dq)
    assert torch.equal(gx, want) and torch.equal(m._model.flat_grad.reshape(-1), dq)
    assert float(dq.abs().max()) > 0
    gx2 = m.backward(ctx, gy, accumulate=True)                            # accumulate= adds to the table gradient
    assert torch.equal(gx2, want)
    assert torch.allclose(m._model.flat_grad.reshape(-1), 2 * dq, rtol=1e-6, atol=0)
    before = m._model.flat.clone()
    m._model.adam(1e-2, 1, 1.0)
    moved = (m._model.flat - before).abs()
    assert float(moved.max()) <= 1.001e-2 and float(moved.mean()) > 1e-3


# ---- 9. dispatcher op -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sub', SUBS)
@pytest.mark.parametrize('rounding', ROUNDINGS)
def test_dispatcher_op_under_autograd(dev, sub, rounding):
    from neural_imaging_amd import ops, torch_ops
    shape = (2, 48, 80)
    hs, vs = FACTORS[sub]
    x = g(S.image(shape, 'saturated'), dev)
    gy = g(C.gradient(shape), dev)
    q = g(S.tables_of(50).astype(np.float32).reshape(3, 8, 8), dev)
    ref = S.reference(sub, shape, 'saturated', 50)
    xr = x.clone().requires_grad_(True)
    qr = q.clone().requires_grad_(True)
    y = torch.ops.nimg.jpeg_ste(xr, qr, rounding, hs, vs)
    y.backward(gy)
    assert torch.equal(y.detach(), g(ref['y'], dev)) and qr.grad is None
    mask = g(ref['mask'], dev)
    want = ops.djpeg_bwd(x, gy, mask, q, rounding) if sub == '4:4:4' else ops.djpeg_sub_bwd(x, gy, mask, q, rounding, hs, vs)
    assert torch.equal(xr.grad, want)
    yr, mr = torch.ops.nimg.jpeg_ste_fwd(x, q, hs, vs)
    assert torch.equal(yr, y.detach()) and torch.equal(mr, mask)
    assert torch.equal(torch_ops.jpeg_ste(x, q, rounding, sub), yr)
    with torch.no_grad():
        assert torch.equal(torch.ops.nimg.jpeg_ste(x, q, rounding, hs, vs), yr)


@pytest.mark.parametrize('sub', SUBS)
def test_graph_capture_replays_the_eager_bits(dev, sub):
    """Forward plus backward, captured on one stream with no side stream: the raw dispatcher ops the Autograd kernel is made of."""
    from neural_imaging_amd import ops, torch_ops  # noqa: F401
    shape = (2, 48, 80)
    hs, vs = FACTORS[sub]
    x = g(S.image(shape, 'saturated'), dev)
    gy = g(C.gradient(shape), dev)
    q = g(S.tables_of(50).astype(np.float32).reshape(3, 8, 8), dev)

    def step():
        y, mask = torch.ops.nimg.jpeg_ste_fwd(x, q, hs, vs)
        gx = torch.ops.nimg.djpeg_bwd(x, gy, mask, q, 'sin') if sub == '4:4:4' else torch.ops.nimg.djpeg_sub_bwd(x, gy, mask, q, 'sin', hs, vs)
        return y, mask, gx
    y_e, mask_e, gx_e = step()
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):                                   # warm-up: the workspace grows outside the capture
        step()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize(dev)
    ops.begin_pin_log()
    graph = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            y, mask, gx = step()
    finally:
        pins = ops.end_pin_log()
    y.zero_(); mask.zero_(); gx.zero_()
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(y, y_e) and torch.equal(mask, mask_e) and torch.equal(gx, gx_e)
    del pins


# ---- 10. workflow ---------------------------------------------------------------------------------------------------------------------------
def test_workflow_trains_through_the_real_codec(dev):
    from neural_imaging_amd.compression.jpeg_helpers import compress_batch
    from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification
    dist = {'downsampling': 'none', 'compression': 'jpeg',
            'compression_params': {'quality': 80, 'codec': 'libjpeg+identity', 'subsampling': '4:2:0'}}
    rgb = natural_images(2, 64, 64, seed=8)
    raw = bayer_from_rgb(rgb)
    losses = []
    for run in range(2):
        np.random.seed(7)
        torch.manual_seed(7)
        wf = ManipulationClassification('UNet', distribution=dist, trainable=('nip',), raw_patch_size=32, device=dev)
        if run == 0:
            state = (wf.nip.state_dict(), wf.fan.state_dict())
            Y, c, C_, ent, probs = wf.run_workflow(raw)
            assert c.shape == (10, 64, 64, 3) and probs.shape == (10, 5)
            real, _ = compress_batch(c.numpy(), 80, subsampling='4:2:0')
            assert np.array_equal(C_.numpy(), np.asarray(real))          # the FAN sees the images of real files
            assert np.array_equal(wf.run_compression(c).numpy(), np.asarray(real))
        else:
            wf.nip.load_state_dict(state[0])
            wf.fan.load_state_dict(state[1])
        before = wf.nip.state_dict()
        np.random.seed(11)
        loss, parts = wf.training_step(raw, rgb, lambda_nip=0.1, learning_rate=1e-4)
        assert np.isfinite(float(loss)) and np.isfinite(float(parts['ce'])) and np.isfinite(float(parts['nip']))
        after = wf.nip.state_dict()
        assert all(not np.array_equal(before[k], after[k]) for k in before), [k for k in before if np.array_equal(before[k], after[k])]
        losses.append(np.float32(float(loss)).tobytes() + np.float32(float(parts['ce'])).tobytes())
    assert losses[0] == losses[1]
