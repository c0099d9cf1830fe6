"""
The operand-preparing kernels every convolution of a step and every batch pass through first, on EVERY route of their dispatch, by
equality (cases, ids and the numpy / Python-integer reference halves: tests/operand_cases.py; its self-test, which also counts the
routes and shows that each comparison fails on a wrong image: tests/test_operand_helpers.py).

Every comparison is assert_bits_equal / assert_exact / np.array_equal / torch.equal; the one exception is the variance of
nimg_patch_stats, held to the DERIVED bound 4 * 2^-53 * exact (three roundings: numerator, denominator, quotient) - its mean must
equal the correctly rounded quotient.  Every output buffer is allocated by the test, 256 bytes larger than needed and pre-filled
with 0xa5: the bytes behind it must come back untouched, and since no reference holds the fill pattern (asserted by the builders)
equality with the reference also says that every element was written.  The entry points are therefore called through _lib with
the test's own buffers; the wrappers of ops.py are checked against those bytes.  Operands: full-mantissa float32 with planted
ties, binade crossings, overflow to inf, +-0, +-inf and a NaN for the bf16 images; all-distinct integers for the permutations;
pixels k / 256 for the affine image; no float32 denormals.

Kernel reached by each test id (read off nimg_* in csrc/conv_bf16.hip, conv_mfma.hip, dgrad5s.hip, latent.hip, datafeed.hip):

  weights_bf16_kernel            wimg-layer-m{0,1}-KHxKW-cinC-coutC-{one-workgroup | several-workgroups | second-trip}: taps 1, 4, 9, 25,
                                 1x3, 3x1; padded axis 3 .. 33; -second-trip = 5x5x160x160 (640 000 elements > 2048 x 256);
                                 wimg-batch-* (every entry again, as the batch kernel's second reference); wimg-registry-* (the
                                 per-layer conversion of every registered parameter and of the unregistered tensor)
  weights_bf16_batch_kernel      wimg-batch-all-N-entries (both modes, rows 1, 63, 64, 65, one tile .. 750 tiles > 384 workgroups),
                                 wimg-batch-n1-more-than-384-tiles, wimg-batch-n1-one-tile, wimg-batch-n40, wimg-batch-arguments;
                                 wimg-registry-{UNet,INet,DNet,FAN,TwitterDCN} (WeightImages.refresh and every entry point's
                                 refresh_images)
  flip_weights_kernel            flip-KHxKW-cinC-coutC (taps 1, 4, 9, 25, 1x3; channels 1, 3, 32, 33), -second-trip (592 128 elements)
  dgrad5s_weights_kernel         dgrad5s-cin{32,64,32}-cout{8,16,64}, dgrad5s-cin128-cout256-second-trip (4.7 M > 8192 x 256),
                                 dgrad5s-arguments
  s2d_conv_weights_kernel        s2dw-cC-cpP-coutK (c 1, 3, 8, 64; cp 4c, 4c + 4, rounded up), s2dw-c64-*-cout128-second-trip
  s2d_conv_weights_bwd_kernel    s2dw-bwd-*-acc{0,1}, s2dw-bwd-c64-cp256-cout192-acc{0,1}-second-trip; every s2dw-* id (bwd(fwd(w5)) == w5)
  s2d2_affine3_bf16_kernel       s2d2-affine3-* (2x2 image, odd block counts), s2d2-affine3-1x1026x1026x3-cp16-ab2-second-trip
  s2d2_affine_bf16_kernel        s2d2-generic-* (c = 3 with cp = 32, c 1, 4, 16, cp > 4c), s2d2-generic-1x260x260x4-cp16-ab2-second-trip
  patch_stats_kernel             stats-p2 / -p10 / -p14 / -p96 / -p1024-*, stats-one-candidate, stats-4096-candidates,
                                 stats-arguments, flat_patches_in_dark_n_textured
  patch_select_kernel            select-<branch> (one lane; ids name the branch of oracle.datafeed.Policy they reach),
                                 select-batch-<mode>-b{1,64,65,130}, select-arguments, flat_patches_in_dark_n_textured
  gather_raw_kernel              gather-every-value-cut-whole, gather-p2-*, gather-p10-*, gather-raw-b9-p1024-second-trip
  gather_rgb_kernel              gather-every-value-cut-whole, gather-p2-*, gather-p10-*, gather-rgb-b6-p512-second-trip

Confirmed by one kernel-trace run of this module (rocprofv3 --kernel-trace --stats, kernel trace alone): all twelve kernels appear.
"""
import functools
import gc
import time

import numpy as np
import pytest
import torch

import operand_cases as C
from util import assert_exact, bayer_from_rgb, natural_images

pytestmark = pytest.mark.gpu

GUARD = C.GUARD
ERR_ARG = -1
_T0 = [None]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    _T0[0] = time.monotonic()
    yield torch.device('cuda', 0)
    print('operands: module wall time {:.1f} s'.format(time.monotonic() - _T0[0]))          # (shown with pytest -s)


def params(cases, prefix=''):
    return [pytest.param(c, id=prefix + c['name']) for c in cases]


def dv(a, dev):
    return torch.from_numpy(np.array(a, order='C')).to(dev).contiguous()          # (np.array: always a copy, writable)


def _guarded(nbytes, dev):
    """(the whole buffer, filled with 0xa5; its first nbytes) - the buffer is checked with _intact afterwards."""
    whole = torch.full((nbytes + GUARD,), C.FILL, dtype=torch.uint8, device=dev)
    assert whole.data_ptr() % 256 == 0
    return whole, whole[:nbytes]


def _intact(whole, nbytes, what):
    assert bool((whole[nbytes:] == C.FILL).all()), 'a write behind ' + what


def _np(view, dtype):
    return view.cpu().numpy().view(dtype)


def _api():
    from neural_imaging_amd import _lib, ops
    return _lib, _lib.load(), ops


# ----------------------------------------------------------------------------------------------------------------------
# 1. bf16 weight images
def _layer_image(w, c, dev):
    """nimg_conv_weights_bf16 into the test's own guarded buffer -> the image bytes (device uint8 tensor)."""
    _lib, lib, ops = _api()
    nbytes = int(lib.nimg_conv_weights_bf16_bytes(c['kh'], c['kw'], c['cin'], c['cout'], c['mode']))
    assert nbytes == C.wimg_bytes(c['kh'], c['kw'], c['cin'], c['cout'], c['mode'])
    whole, out = _guarded(nbytes, dev)
    _lib.call('nimg_conv_weights_bf16', ops._p(w), ops._p(out), c['kh'], c['kw'], c['cin'], c['cout'], c['mode'], ops._stream())
    _intact(whole, nbytes, 'the weight image')
    return out


@functools.lru_cache(maxsize=None)
def _wimg(kh, kw, cin, cout, mode):
    return C.wimg_case(dict(kh=kh, kw=kw, cin=cin, cout=cout, mode=mode, name='wimg {}x{}x{}x{} m{}'.format(kh, kw, cin, cout, mode)))


@pytest.mark.parametrize('case', params(C.WIMG_LAYER_CASES))
def test_weight_image_layer(dev, case):
    _lib, lib, ops = _api()
    r = _wimg(case['kh'], case['kw'], case['cin'], case['cout'], case['mode'])
    w = dv(r['w'], dev)
    out = _layer_image(w, case, dev)
    C.assert_bits_equal(_np(out, np.uint16), r['ref'], case['name'])
    assert torch.equal(ops.weights_bf16(w, case['mode']), out), 'ops.weights_bf16 (unregistered path)'


@pytest.mark.parametrize('case', params(C.WIMG_BATCH_CASES))
def test_weight_image_batch(dev, case):
    """One table, both modes, 256-byte aligned slots with 0xa5 gaps: every image equals the reference AND the per-layer kernel's
    bytes; the gaps and the guard survive."""
    _lib, lib, ops = _api()
    entries = C.batch_entries(case)
    assert len(entries) == case['n']
    refs = [_wimg(e['kh'], e['kw'], e['cin'], e['cout'], e['mode']) for e in entries]
    sizes = [r['ref'].size * 2 for r in refs]
    offs, total = C.batch_layout(sizes)
    whole, buf = _guarded(total, dev)
    ws = [dv(r['w'], dev) for r in refs]
    table = np.zeros((len(entries), 4), np.int64)
    for i, (e, w) in enumerate(zip(entries, ws)):
        table[i] = (w.data_ptr(), buf.data_ptr() + offs[i], ((e['kh'] * e['kw']) << 32) | e['mode'], (e['cin'] << 32) | e['cout'])
    tab = dv(table, dev)
    _lib.call('nimg_conv_weights_bf16_batch', ops._p(tab), len(entries), ops._stream())
    _intact(whole, total, 'the image buffer')
    got = buf.cpu().numpy()
    gap = np.ones(total, bool)
    for i, (e, r) in enumerate(zip(entries, refs)):
        C.assert_bits_equal(got[offs[i]:offs[i] + sizes[i]].view(np.uint16), r['ref'], '{} entry {} ({}, {} tiles)'.format(
            case['name'], i, e['name'], e['tiles']))
        assert torch.equal(buf[offs[i]:offs[i] + sizes[i]], _layer_image(ws[i], e, dev)), 'entry {} ({}) differs from the per-layer kernel'.format(i, e['name'])
        gap[offs[i]:offs[i] + sizes[i]] = False
    assert gap.sum() >= 256 * len(entries) and (got[gap] == C.FILL).all(), 'a write into the gap between two slots'


def test_weight_image_batch_arguments(dev):
    """wimg-batch-arguments: n_entries = 0 is OK with a null table; a negative count or a null table is NIMG_ERR_ARG."""
    _lib, lib, ops = _api()
    tab = torch.zeros(4, dtype=torch.int64, device=dev)
    s = ops._stream()
    assert lib.nimg_conv_weights_bf16_batch(None, 0, s) == 0 and lib.nimg_conv_weights_bf16_batch(ops._p(tab), 0, s) == 0
    assert lib.nimg_conv_weights_bf16_batch(None, 1, s) == ERR_ARG and lib.nimg_conv_weights_bf16_batch(ops._p(tab), -1, s) == ERR_ARG
    assert lib.nimg_conv_weights_bf16_batch(None, -1, s) == ERR_ARG
    w, (whole, out) = torch.ones(16, device=dev), _guarded(64, dev)
    for bad in ((0, 1, 1, 1, 0), (1, 1, 0, 1, 0), (1, 1, 1, 0, 0), (1, 1, 1, 1, 2), (1, 1, 1, 1, -1)):
        assert lib.nimg_conv_weights_bf16(ops._p(w), ops._p(out), *bad, s) == ERR_ARG
    assert lib.nimg_conv_weights_bf16(None, ops._p(out), 1, 1, 1, 1, 0, s) == ERR_ARG
    torch.cuda.synchronize()
    _intact(whole, 0, 'a refused call')


# ---- ops.WeightImages and the registry
def _families():
    from neural_imaging_amd.models import compression, forensics, pipelines
    rgb = natural_images(4, 64, 64, seed=41)
    raw = bayer_from_rgb(rgb)
    return {'UNet': (lambda d: pipelines.UNet(patch_size=32, device=d), raw, ('forward', 'process')),
            'INet': (lambda d: pipelines.INet(patch_size=32, random_init=True, device=d), raw, ('forward', 'process')),
            'DNet': (lambda d: pipelines.DNet(patch_size=32, n_layers=4, n_features=16, device=d), raw, ('forward', 'process')),
            'FAN': (lambda d: forensics.FAN(n_classes=5, patch_size=64, device=d), rgb, ('forward', 'process')),
            'TwitterDCN': (lambda d: compression.TwitterDCN(patch_size=64, n_features=8, device=d), rgb,
                           ('forward', 'process', 'encode', 'decode'))}


def _params4(net):
    return [(k, p) for k, p in net._model.p.items() if p.dim() == 4 and min(p.shape) > 0]


def _check_images(net, dev, what):
    """Every registered view == the per-layer conversion of the parameter as it is NOW into a fresh buffer; the rest of the model's
    image buffer is still 0xa5."""
    _lib, lib, ops = _api()
    images = net._model.images
    base, size = images.buf.data_ptr(), images.buf.numel()
    gap = torch.ones(size, dtype=torch.bool, device=dev)
    for name, p in _params4(net):
        kh, kw, cin, cout = p.shape
        for mode in (0, 1):
            view = ops.weights_bf16(p, mode)
            off = view.data_ptr() - base
            assert 0 <= off and off + view.numel() <= size and off % 256 == 0, name
            fresh = _layer_image(p, dict(kh=kh, kw=kw, cin=cin, cout=cout, mode=mode), dev)
            assert view.numel() == fresh.numel() and torch.equal(view, fresh), '{}: image of {} (mode {}) is not the conversion of its weights'.format(what, name, mode)
            gap[off:off + view.numel()] = False
    assert bool((images.buf[gap] == C.FILL).all()), what + ': a write into an alignment gap'


def _registry_walk(family, dev):
    """Everything that needs the model alive; -> (base, size) of its image buffer, (pointer, shape) of its 4-D parameters."""
    _lib, lib, ops = _api()
    make, x_np, entry_points = _families()[family]
    net = make(dev)
    images = net._model.images
    p4 = _params4(net)
    assert len(p4) >= 1 and len(images.entries) == 2 * len(p4)
    base, size = images.buf.data_ptr(), images.buf.numel()
    for name, p in p4:                                        # (this includes the 2x2 transposed kernels and the constrained filter)
        for mode in (0, 1):
            view = ops.weights_bf16(p, mode)
            assert view.data_ptr() == ops._WB_REGISTRY[p.data_ptr()][mode].data_ptr() and base <= view.data_ptr() < base + size, name
            assert view.numel() == C.wimg_bytes(*p.shape, mode)
    if family == 'UNet':
        assert any(tuple(p.shape[:2]) == (2, 2) for _, p in p4), 'no transposed-convolution kernel among the registered'
    if family == 'FAN':
        assert any(p.shape[2] == 3 and p.shape[3] == 3 for _, p in p4), 'the 3-channel constrained filter is not registered'
    images.buf.fill_(C.FILL)
    images.refresh()
    _check_images(net, dev, family + ' refresh()')
    # every entry point rebuilds the images from the weights as they are when it is called
    x = dv(x_np, dev)
    lat = net.encode(x)[0] if 'decode' in entry_points else None
    for k, entry in enumerate(entry_points):
        rng = np.random.default_rng(100 + k)
        state = {key: (v * (1 + 0.01 * rng.standard_normal(v.shape))).astype(np.float32) for key, v in net.state_dict().items()}
        net.load_state_dict(state)
        images.buf.fill_(C.FILL)
        if entry == 'process':
            net.process(x_np)
        elif entry == 'decode':
            net.decode(lat)
        else:
            getattr(net, entry)(x)
        _check_images(net, dev, '{}.{}() after load_state_dict'.format(family, entry))
    # parity mode: refresh() leaves the buffer alone
    ops.set_compute('f32')
    images.buf.fill_(C.FILL)
    images.refresh()
    net._model.refresh_images()
    assert bool((images.buf == C.FILL).all()), 'refresh() wrote images with COMPUTE == f32'
    ops.set_compute('bf16')
    # a fresh tensor of a registered shape goes through the unregistered path
    name, p = p4[0]
    fresh_w = p.clone()
    assert fresh_w.data_ptr() not in ops._WB_REGISTRY
    img = ops.weights_bf16(fresh_w, 0)
    assert not (base <= img.data_ptr() < base + size)
    kh, kw, cin, cout = p.shape
    assert torch.equal(img, _layer_image(p, dict(kh=kh, kw=kw, cin=cin, cout=cout, mode=0), dev))
    return (base, size), [(p.data_ptr(), tuple(p.shape)) for _, p in p4]


@pytest.mark.parametrize('family', ['UNet', 'INet', 'DNet', 'FAN', 'TwitterDCN'], ids=lambda f: 'wimg-registry-' + f)
def test_weight_images_registry(dev, family):
    _lib, lib, ops = _api()
    ops.set_compute('bf16')
    try:
        (base, size), keys = _registry_walk(family, dev)
    finally:
        ops.set_compute('f32')
    gc.collect()
    for ptr, reg in list(ops._WB_REGISTRY.items()):
        for mode in (0, 1):
            assert mode not in reg or not (base <= reg[mode].data_ptr() < base + size), \
                'a registry entry ({:#x}, {}) points into the image buffer of a model that is gone'.format(ptr, reg['shape'])


# ----------------------------------------------------------------------------------------------------------------------
# 2. nimg_conv_flip_weights
@pytest.mark.parametrize('case', params(C.FLIP_CASES))
def test_flip_weights(dev, case):
    _lib, lib, ops = _api()
    r = C.flip_case(case)
    kh, kw, cin, cout = r['w'].shape
    w = dv(r['w'], dev)
    whole, out = _guarded(4 * r['w'].size, dev)
    _lib.call('nimg_conv_flip_weights', ops._p(w), ops._p(out), kh, kw, cin, cout, ops._stream())
    _intact(whole, 4 * r['w'].size, 'the flipped weights')
    assert_exact(_np(out, np.float32).reshape(kh, kw, cout, cin), r['ref'], case['name'])
    wt = ops.flip_weights(w)
    assert wt.shape == (kh, kw, cout, cin) and torch.equal(wt.reshape(-1), out.view(torch.float32))
    dst = torch.full((kh, kw, cout, cin), 7.0, device=dev)
    assert ops.flip_weights(w, out=dst) is dst and torch.equal(dst, wt), 'the out= form'
    assert torch.equal(ops.flip_weights(wt), w), 'flipping twice with the channel roles swapped is not the identity'


# ----------------------------------------------------------------------------------------------------------------------
# 3. the 2:4 sparse input-gradient image
@pytest.mark.parametrize('case', params(C.DGRAD5S_CASES))
def test_dgrad5s_weight_image(dev, case):
    _lib, lib, ops = _api()
    r = C.dgrad5s_case(case)
    cin, cout = case['cin'], case['cout']
    nbytes = int(lib.nimg_conv5_dgrad_sparse_image_bytes(cin, cout))
    assert nbytes == r['ref'].size * 2 == C.dgrad5s_image_bytes(cin, cout)
    whole, out = _guarded(nbytes, dev)
    w = dv(r['w'], dev)
    _lib.call('nimg_conv5_dgrad_sparse_weights', ops._p(w), ops._p(out), cin, cout, ops._stream())
    _intact(whole, nbytes, 'the sparse image')
    C.assert_bits_equal(_np(out, np.uint16), r['ref'], case['name'])


def test_dgrad5s_weight_image_arguments(dev):
    _lib, lib, ops = _api()
    w, (whole, out) = torch.ones(25 * 64 * 64, device=dev), _guarded(1024, dev)
    for cin, cout in C.DGRAD5S_REFUSED:
        assert int(lib.nimg_conv5_dgrad_sparse_image_bytes(cin, cout)) == 0 == C.dgrad5s_image_bytes(cin, cout)
        assert lib.nimg_conv5_dgrad_sparse_weights(ops._p(w), ops._p(out), cin, cout, ops._stream()) == ERR_ARG
    assert lib.nimg_conv5_dgrad_sparse_weights(None, ops._p(out), 32, 8, ops._stream()) == ERR_ARG
    torch.cuda.synchronize()
    _intact(whole, 0, 'a refused call')


# ----------------------------------------------------------------------------------------------------------------------
# 4. space-to-depth builders
@pytest.mark.parametrize('case', params(C.S2DW_CASES))
def test_s2d_conv_weights(dev, case):
    _lib, lib, ops = _api()
    r = C.s2dw_case(case)
    c, cp, cout = case['c'], case['cp'], case['cout']
    w5 = dv(r['w5'], dev)
    nbytes = 9 * cp * cout * 4
    whole, out = _guarded(nbytes, dev)
    _lib.call('nimg_s2d_conv_weights', ops._p(w5), ops._p(out), c, cp, cout, ops._stream())
    _intact(whole, nbytes, 'w3')
    assert_exact(_np(out, np.float32).reshape(3, 3, cp, cout), r['ref'], case['name'])
    w3 = ops.s2d_conv_weights(w5, cp=cp)
    assert torch.equal(w3.reshape(-1), out.view(torch.float32))
    if cp == C.ceil16(4 * c):
        assert torch.equal(ops.s2d_conv_weights(w5), w3), 'the default cp'
    back = torch.full((5, 5, c, cout), 7.0, device=dev)
    ops.s2d_conv_weights_bwd(w3, back)
    assert torch.equal(back, w5), 'bwd(fwd(w5)) != w5'


@pytest.mark.parametrize('case', params(C.S2DW_BWD_CASES))
def test_s2d_conv_weights_bwd(dev, case):
    _lib, lib, ops = _api()
    r = C.s2dw_bwd_case(case)
    c, cp, cout = case['c'], case['cp'], case['cout']
    dw3 = dv(r['dw3'], dev)
    nbytes = 25 * c * cout * 4
    whole, out = _guarded(nbytes, dev)
    if case['acc']:
        out.view(torch.float32).copy_(dv(r['existing'], dev).reshape(-1))
    _lib.call('nimg_s2d_conv_weights_bwd', ops._p(dw3), ops._p(out), c, cp, cout, case['acc'], ops._stream())
    _intact(whole, nbytes, 'dw5')
    assert_exact(_np(out, np.float32).reshape(5, 5, c, cout), r['ref'], case['name'])
    dw5 = dv(r['existing'], dev)
    assert ops.s2d_conv_weights_bwd(dw3, dw5, accumulate=bool(case['acc'])) is dw5
    assert torch.equal(dw5.reshape(-1), out.view(torch.float32))


def test_s2d_conv_weights_arguments(dev):
    """cp < 4 c is refused by the wrapper and by the entry points."""
    _lib, lib, ops = _api()
    w5, w3 = torch.ones((5, 5, 3, 2), device=dev), torch.ones((3, 3, 8, 2), device=dev)
    s = ops._stream()
    assert lib.nimg_s2d_conv_weights(ops._p(w5), ops._p(w3), 3, 8, 2, s) == ERR_ARG
    assert lib.nimg_s2d_conv_weights_bwd(ops._p(w3), ops._p(w5), 3, 8, 2, 0, s) == ERR_ARG
    assert lib.nimg_s2d_conv_weights(ops._p(w5), ops._p(w3), 0, 8, 2, s) == ERR_ARG and lib.nimg_s2d_conv_weights(None, ops._p(w3), 2, 8, 2, s) == ERR_ARG
    with pytest.raises(ValueError):
        ops.s2d_conv_weights_bwd(w3, w5)
    with pytest.raises(RuntimeError):
        ops.s2d_conv_weights(w5, cp=8)
    with pytest.raises(ValueError):
        ops.s2d_conv_weights(torch.ones((3, 3, 3, 2), device=dev))
    torch.cuda.synchronize()
    assert bool((w5 == 1).all()) and bool((w3 == 1).all())


@pytest.mark.parametrize('case', params(C.AFFINE_CASES))
def test_s2d2_affine(dev, case):
    _lib, lib, ops = _api()
    r = C.affine_case(case)
    n, h, w, c, cp = case['n'], case['h'], case['w'], case['c'], case['cp']
    x = dv(r['x'], dev)
    nbytes = r['ref'].size * 2
    whole, out = _guarded(nbytes, dev)
    _lib.call('nimg_s2d2_affine_bf16', ops._p(x), ops._p(out), n, h, w, c, cp, float(r['a']), float(r['b']), ops._stream())
    _intact(whole, nbytes, 'the space-to-depth image')
    got = _np(out, np.uint16).reshape(r['ref'].shape)
    C.assert_bits_equal(got, r['ref'], case['name'])
    assert not got[..., 4 * c:].any(), 'padding channels must be +0.0, bit for bit'
    y = ops.s2d2_affine(x, r['a'], r['b'], cp=cp)
    assert y.dtype == torch.bfloat16 and torch.equal(y.view(torch.int16).reshape(-1), out.view(torch.int16))
    if c == 3 and cp == 32:                     # the same data through the other route: the first 16 block channels are affine3's image
        y16 = ops.s2d2_affine(x, r['a'], r['b'])
        assert y16.shape[-1] == 16 and torch.equal(y16.view(torch.int16), y.view(torch.int16)[..., :16])


def test_s2d2_affine_arguments(dev):
    _lib, lib, ops = _api()
    x, (whole, out) = torch.ones(3 * 4 * 3, device=dev), _guarded(256, dev)
    s = ops._stream()
    for n, h, w, c, cp in ((1, 3, 4, 3, 16), (1, 4, 3, 3, 16), (1, 3, 4, 1, 4), (1, 2, 2, 3, 8), (1, 2, 2, 0, 4), (-1, 2, 2, 3, 16)):
        assert lib.nimg_s2d2_affine_bf16(ops._p(x), ops._p(out), n, h, w, c, cp, 1.0, 0.0, s) == ERR_ARG, (n, h, w, c, cp)
    assert lib.nimg_s2d2_affine_bf16(None, None, 0, 2, 2, 3, 16, 1.0, 0.0, s) == 0
    with pytest.raises(RuntimeError):
        ops.s2d2_affine(torch.ones((1, 3, 4, 3), device=dev))
    with pytest.raises(RuntimeError):
        ops.s2d2_affine(torch.ones((1, 4, 5, 3), device=dev))
    torch.cuda.synchronize()
    _intact(whole, 0, 'a refused call')


# ----------------------------------------------------------------------------------------------------------------------
# 5. data feed
def _stats(ops, _lib, dev, rgb_t, n, h, w, idx, cand, p):
    b, attempts = cand.shape[0], cand.shape[1]
    nbytes = 8 * b * attempts
    (vw, var), (mw, mean) = _guarded(nbytes, dev), _guarded(nbytes, dev)
    idx_t, cand_t = dv(idx, dev), dv(cand, dev)                 # (held in names: a temporary would be freed before the launch)
    assert int(idx.max()) < n and int(idx.min()) >= 0
    _lib.call('nimg_patch_stats', ops._p(rgb_t), n, h, w, ops._p(idx_t), ops._p(cand_t), b, attempts, p, ops._p(var),
              ops._p(mean), ops._stream())
    _intact(vw, nbytes, 'var')
    _intact(mw, nbytes, 'mean')
    return _np(var, np.float64).reshape(b, attempts), _np(mean, np.float64).reshape(b, attempts), var, mean


@pytest.mark.parametrize('case', params(C.STATS_CASES))
def test_patch_stats(dev, case):
    """mean == float(Fraction(S, 255 n)); |var - exact| <= 4 * 2^-53 * exact (derived: three roundings); flat patch: var == 0.0."""
    _lib, lib, ops = _api()
    r = C.stats_case(case)
    rgb, idx, cand, p = r['rgb'], r['image_idx'], r['cand'], case['p']
    n, h, w, _ = rgb.shape
    rgb_t = dv(rgb, dev)
    var, mean, var_t, mean_t = _stats(ops, _lib, dev, rgb_t, n, h, w, idx, cand, p)
    assert not (var.view(np.uint64) == 0xa5a5a5a5a5a5a5a5).any() and not (mean.view(np.uint64) == 0xa5a5a5a5a5a5a5a5).any(), 'unwritten'
    worst, flat = 0.0, 0
    for i in range(case['b']):
        for k in range(case['attempts']):
            xx, yy = int(cand[i, k, 0]), int(cand[i, k, 1])
            C.assert_stats(var[i, k], mean[i, k], rgb[idx[i]], xx, yy, p, '{} candidate ({}, {})'.format(case['name'], i, k))
            exact = C.stats_reference(rgb[idx[i]], xx, yy, p)[1]
            flat += exact == 0
            if exact:
                worst = max(worst, float(abs(C.Fraction(float(var[i, k])) - exact) / exact) * 2.0 ** 53)
    print('{}: worst |var - exact| / exact = {:.3f} x 2^-53 (bound 4), {} exactly flat patches'.format(case['name'], worst, flat))
    if case['images'] != 'square96' and case['b'] >= 3:
        assert flat >= 1
    v2, m2 = ops.patch_stats(rgb_t, dv(idx, dev), dv(cand, dev), p)
    assert torch.equal(v2.reshape(-1), var_t.view(torch.float64)) and torch.equal(m2.reshape(-1), mean_t.view(torch.float64))


def test_patch_stats_arguments(dev):
    """stats-arguments: odd patch, patch > h, patch 1026, attempts <= 0, ODD h or w (as nimg_patch_gather refuses them) -> NIMG_ERR_ARG;
    b = 0 -> OK with null buffers."""
    _lib, lib, ops = _api()
    rgb = torch.zeros((1, 1030, 1030, 3), dtype=torch.uint8, device=dev)
    idx, cand = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 1, 2), dtype=torch.int32, device=dev)
    (vw, var), (mw, mean) = _guarded(8, dev), _guarded(8, dev)
    s = ops._stream()

    def call(h, w, b, attempts, patch, null=False):
        if null:
            return lib.nimg_patch_stats(None, 1, h, w, None, None, b, attempts, patch, None, None, s)
        return lib.nimg_patch_stats(ops._p(rgb), 1, h, w, ops._p(idx), ops._p(cand), b, attempts, patch, ops._p(var), ops._p(mean), s)

    assert call(1030, 1030, 1, 1, 1024) == 0
    for h, w, b, attempts, patch in ((1030, 1030, 1, 1, 3), (16, 1030, 1, 1, 18), (1030, 16, 1, 1, 18), (1030, 1030, 1, 1, 1026),
                                     (1030, 1030, 1, 0, 2), (1030, 1030, 1, -1, 2), (1030, 1030, -1, 1, 2), (1030, 1030, 1, 1, 0),
                                     (1030, 1029, 1, 1, 2), (1029, 1030, 1, 1, 2), (11, 11, 1, 1, 2)):
        assert call(h, w, b, attempts, patch) == ERR_ARG, (h, w, b, attempts, patch)
    assert call(1030, 1030, 0, 1, 2, null=True) == 0
    assert call(1030, 1030, 1, 1, 2, null=True) == ERR_ARG
    with pytest.raises(RuntimeError):                          # ops.patch_stats raises on the status: an odd width
        ops.patch_stats(torch.zeros((1, 10, 11, 3), dtype=torch.uint8, device=dev), idx, cand, 2)
    with pytest.raises(RuntimeError):
        ops.patch_stats(torch.zeros((1, 11, 10, 3), dtype=torch.uint8, device=dev), idx, cand, 2)
    torch.cuda.synchronize()
    _intact(vw, 8, 'var')
    _intact(mw, 8, 'mean')


def _select(ops, _lib, dev, mode, cand, var, mean, uni, max_attempts, want_used=True):
    """nimg_patch_select on hand-built statistics, through _lib with guarded outputs; statistics are null in mode 0 and the
    uniforms are null outside 'flat'.  -> (chosen_xy as a list, attempts_used as a list | None)."""
    from oracle import datafeed as odf
    b, attempts = cand.shape[0], cand.shape[1]
    (xw, xy), (uw, used) = _guarded(8 * b, dev), _guarded(4 * b, dev)
    var_t = dv(var, dev) if mode else None
    mean_t = dv(mean, dev) if mode else None
    uni_t = dv(uni, dev) if mode == 'flat' else None
    cand_t = dv(cand, dev)
    _lib.call('nimg_patch_select', ops._p(cand_t), ops._p(uni_t), ops._p(var_t), ops._p(mean_t), b, attempts, max_attempts,
              odf.MODES[mode], ops._p(xy), ops._p(used) if want_used else None, ops._stream())
    _intact(xw, 8 * b, 'chosen_xy')
    _intact(uw, 4 * b if want_used else 0, 'attempts_used')
    return _np(xy, np.int32).reshape(b, 2).tolist(), (_np(used, np.int32).tolist() if want_used else None)


@pytest.mark.parametrize('case', params(C.SELECT_CASES, 'select-'))
def test_patch_select_branch(dev, case):
    """One lane on designed float64 statistics: the kernel and oracle.datafeed.Policy make the same float64 comparisons, so the
    answers must be identical - no margin.  The builder asserts on the oracle that the case reaches the branch its id names."""
    _lib, lib, ops = _api()
    r = C.select_case(case)
    xy, used = _select(ops, _lib, dev, case['mode'], r['cand'], r['var'], r['mean'], r['uni'], case['max_attempts'])
    assert xy == [r['want_xy']] and used == [r['want_used']], '{}: device {} after {}, oracle {} after {}'.format(
        case['name'], xy, used, r['want_xy'], r['want_used'])
    xy2, none = _select(ops, _lib, dev, case['mode'], r['cand'], r['var'], r['mean'], r['uni'], case['max_attempts'], want_used=False)
    assert xy2 == xy and none is None                                   # attempts_used = NULL


@pytest.mark.parametrize('b', C.SELECT_BATCH_SIZES, ids=lambda b: 'b{}'.format(b))
@pytest.mark.parametrize('mode', [None, 'flat', 'flat-aggressive', 'dark-n-textured'], ids=lambda m: 'select-batch-{}'.format(m or 'none'))
def test_patch_select_batch(dev, mode, b):
    """b = 1, 64, 65, 130: the lane guard of the last 64-lane workgroup; every lane walks another designed case."""
    _lib, lib, ops = _api()
    r = C.select_batch(mode, b)
    xy, used = _select(ops, _lib, dev, mode, r['cand'], r['var'], r['mean'], r['uni'], 3)
    assert xy == r['want_xy'] and used == r['want_used']
    if mode:
        xy3, used3 = ops.patch_select(dv(r['cand'], dev), dv(r['uni'], dev), dv(r['var'], dev), dv(r['mean'], dev), mode, 3)
        assert xy3.cpu().numpy().tolist() == xy and used3.cpu().numpy().tolist() == used


def test_patch_select_arguments(dev):
    """select-arguments: mode 4, max_attempts = 0, null var with a mode, null uniforms with 'flat' -> NIMG_ERR_ARG; b = 0 -> OK."""
    _lib, lib, ops = _api()
    cand = torch.zeros((1, 2, 2), dtype=torch.int32, device=dev)
    stat, uni = torch.zeros((1, 2), dtype=torch.float64, device=dev), torch.zeros((1, 2), dtype=torch.float32, device=dev)
    (xw, xy), (uw, used) = _guarded(8, dev), _guarded(4, dev)
    s = ops._stream()

    def call(var, mean, u, b, attempts, max_attempts, mode, c=cand, out=xy):
        return lib.nimg_patch_select(ops._p(c), ops._p(u), ops._p(var), ops._p(mean), b, attempts, max_attempts, mode, ops._p(out),
                                     ops._p(used), s)

    assert call(stat, stat, uni, 1, 2, 1, 4) == ERR_ARG and call(stat, stat, uni, 1, 2, 1, -1) == ERR_ARG
    assert call(stat, stat, uni, 1, 2, 0, 1) == ERR_ARG and call(stat, stat, uni, 1, 0, 1, 1) == ERR_ARG
    for mode in (1, 2, 3):
        assert call(None, stat, uni, 1, 2, 1, mode) == ERR_ARG and call(stat, None, uni, 1, 2, 1, mode) == ERR_ARG
    assert call(stat, stat, None, 1, 2, 1, 1) == ERR_ARG
    assert call(stat, stat, uni, 1, 2, 1, 1, c=None) == ERR_ARG and call(stat, stat, uni, 1, 2, 1, 1, out=None) == ERR_ARG
    assert call(None, None, None, 0, 2, 1, 1, c=None, out=None) == 0
    torch.cuda.synchronize()
    _intact(xw, 0, 'a refused call')
    _intact(uw, 0, 'a refused call')
    assert call(stat, stat, None, 1, 2, 1, 2) == 0 and call(stat, stat, None, 1, 2, 1, 3) == 0 and call(None, None, None, 1, 2, 1, 0) == 0


def test_flat_patches_in_dark_n_textured(dev):
    """Real, exactly flat images at levels 128, 200 and 150 (means inside (0.35, 0.99)).  The device's variance is exactly 0.0 and
    'dark-n-textured' rejects the patch by `0 < v`, as the reference's condition reads; the reference's np.var is a positive rounding
    residue at 200 and 150 (and 0 at 128), so the ORACLE accepts those patches.  Both choices are pinned here side by side - the
    documented deviation of nimg_patch_select (csrc/datafeed.hip, include/nimg.h, oracle/datafeed.py)."""
    _lib, lib, ops = _api()
    r = C.flat_patch_case()
    rgb, idx, cand, p = r['rgb'], r['image_idx'], r['cand'], r['p']
    n, h, w, _ = rgb.shape
    var, mean, _, _ = _stats(ops, _lib, dev, dv(rgb, dev), n, h, w, idx, cand, p)
    for i in range(4):
        for k in range(3):
            C.assert_stats(var[i, k], mean[i, k], rgb[idx[i]], int(cand[i, k, 0]), int(cand[i, k, 1]), p)
    assert (var[:3] == 0.0).all() and (var[3, :2] == 0.0).all() and 0 < var[3, 2] < 0.005
    for ma in (2, 3):
        xy, used = _select(ops, _lib, dev, 'dark-n-textured', cand, var, mean, np.zeros((4, 3), np.float32), ma)
        oracle = r['oracle'][ma]
        print('max_attempts {}: device {} after {}; oracle {} after {}'.format(ma, xy, used, [list(o[0]) for o in oracle], [o[1] for o in oracle]))
        assert xy == r['device'][ma]['xy'] and used == r['device'][ma]['used']
        assert used[0] == oracle[0][1] and xy[0] == list(oracle[0][0])                   # level 128: np.var is 0 as well - they agree
        assert all(used[i] != oracle[i][1] for i in (1, 2, 3))                            # levels 200, 150: the oracle took candidate 0
    assert r['device'][3]['xy'][3] != list(r['oracle'][3][3][0])


@pytest.mark.parametrize('case', params(C.GATHER_CASES))
def test_patch_gather(dev, case):
    _lib, lib, ops = _api()
    r = C.gather_case(case)
    b, p = case['b'], case['p']
    raw_t = None if r['raw'] is None else dv(r['raw'].view(np.int16), dev)
    rgb_t = None if r['rgb'] is None else dv(r['rgb'], dev)
    idx_t, xy_t = dv(r['image_idx'], dev), dv(r['xy'], dev)
    xb, yb = b * (p // 2) ** 2 * 16, b * p * p * 12
    (xw, x), (yw, y) = (_guarded(xb, dev) if raw_t is not None else (None, None)), (_guarded(yb, dev) if rgb_t is not None else (None, None))
    _lib.call('nimg_patch_gather', ops._p(raw_t), ops._p(rgb_t), r['n'], r['h'], r['w'], ops._p(idx_t), ops._p(xy_t), b, p, ops._p(x),
              ops._p(y), ops._stream())
    if x is not None:
        _intact(xw, xb, 'x_out')
        assert np.array_equal(_np(x, np.float32).reshape(r['x'].shape), r['x']), case['name'] + ': RAW crop'
    if y is not None:
        _intact(yw, yb, 'y_out')
        assert np.array_equal(_np(y, np.float32).reshape(r['y'].shape), r['y']), case['name'] + ': RGB crop'
    if b <= 5:
        x2, y2 = ops.patch_gather(raw_t, rgb_t, idx_t, xy_t, p)
        assert (x2 is None) == (x is None) and (x is None or torch.equal(x2.reshape(-1), x.view(torch.float32)))
        assert (y2 is None) == (y is None) and (y is None or torch.equal(y2.reshape(-1), y.view(torch.float32)))


def test_patch_gather_arguments(dev):
    """Odd patch, h or w; an output requested without its source; no output at all -> NIMG_ERR_ARG; b = 0 -> OK."""
    _lib, lib, ops = _api()
    raw = torch.zeros((1, 8, 8, 4), dtype=torch.int16, device=dev)
    rgb = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=dev)
    idx, xy = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros((1, 2), dtype=torch.int32, device=dev)
    (xw, x), (yw, y) = _guarded(4 * 4 * 16, dev), _guarded(8 * 8 * 12, dev)
    s = ops._stream()

    def call(raw_, rgb_, h, w, b, patch, x_, y_):
        return lib.nimg_patch_gather(ops._p(raw_), ops._p(rgb_), 1, h, w, ops._p(idx), ops._p(xy), b, patch, ops._p(x_), ops._p(y_), s)

    for args in ((raw, rgb, 16, 16, 1, 7, x, y), (raw, rgb, 15, 16, 1, 8, x, y), (raw, rgb, 16, 15, 1, 8, x, y), (raw, rgb, 16, 16, 1, 18, x, y),
                 (None, rgb, 16, 16, 1, 8, x, y), (raw, None, 16, 16, 1, 8, x, y), (raw, rgb, 16, 16, 1, 8, None, None),
                 (raw, rgb, 16, 16, -1, 8, x, y), (raw, rgb, 16, 16, 1, 0, x, y)):
        assert call(*args) == ERR_ARG, args[2:6]
    assert call(None, None, 16, 16, 0, 8, None, None) == 0
    torch.cuda.synchronize()
    _intact(xw, 0, 'a refused call')
    _intact(yw, 0, 'a refused call')
    assert call(raw, rgb, 16, 16, 1, 8, x, y) == 0
    torch.cuda.synchronize()
    assert not _np(x, np.float32).any() and not _np(y, np.float32).any()
