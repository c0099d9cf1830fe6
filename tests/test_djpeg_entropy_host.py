"""The dJPEG rate term without a GPU: the model surface of JPEG(entropy_weight=), the default model and workflow
unchanged, the error codes the C ABI returns before any launch, and the five-centre window bound the kernels rest on."""
import ctypes

import numpy as np
import pytest
import torch

import djpeg_entropy_ref as R

ERR_ARG, ERR_WORKSPACE = -1, -3


def test_constructor_rules_refusals_and_repr():
    from neural_imaging_amd.models import jpeg
    j = jpeg.JPEG(60, 'sin', trainable=True, device='cpu', entropy_weight=0.25)
    assert j.entropy_weight == 0.25 and j.count_parameters() == 128
    assert repr(j) == 'JPEG(quality=60,codec="sin",trainable=True,entropy_weight=0.25)'
    assert j.summary().startswith('JPEG (sin) trainable QF~') and j.summary().endswith(' H+0.25')
    assert jpeg.JPEG(80, 'harmonic', device='cpu', entropy_weight=0).entropy_weight == 0.0       # zero: reported, no gradient
    assert jpeg.JPEG(80, 'soft', device='cpu', entropy_weight=2).summary() == 'JPEG (soft) QF=80 H+2.0'
    assert jpeg.JPEG(80, 'soft', device='cpu', entropy_weight=2).summary_compact() == 'JPEG (soft) QF=80 H+2.0'
    assert repr(jpeg.JPEG(80, 'soft', device='cpu', subsampling='4:4:4', entropy_weight=1.5)) == \
        'JPEG(quality=80,codec="soft",trainable=False,entropy_weight=1.5)'
    for bad in (-1.0, float('nan'), 'a lot', True):
        with pytest.raises(ValueError):
            jpeg.JPEG(80, 'sin', device='cpu', entropy_weight=bad)
    with pytest.raises(ValueError):
        jpeg.JPEG(80, 'libjpeg', device='cpu', entropy_weight=1.0)          # no gradient, and its rate is real bytes
    for sub in ('4:2:2', '4:2:0'):
        with pytest.raises(ValueError):
            jpeg.JPEG(80, 'sin', device='cpu', subsampling=sub, entropy_weight=1.0)
    # entropy_weight is the last keyword: the positional order of the constructor is unchanged
    import inspect
    assert list(inspect.signature(jpeg.JPEG.__init__).parameters)[1:] == ['quality', 'codec', 'trainable', 'device', 'subsampling',
                                                                          'entropy_weight']
    assert list(inspect.signature(jpeg.JPEG.backward).parameters)[1:] == ['ctx', 'dy', 'accumulate', 'entropy_coef']
    with pytest.raises(ValueError):                                         # a rate gradient needs the ctx of a rate model
        jpeg.JPEG.backward(_NoDistortion(j), {'learned': False}, None, entropy_coef=1.0)


class _NoDistortion(object):
    """JPEG.backward with the distortion kernels (GPU) stubbed out: only the rate branch's own refusal is looked at."""

    def __init__(self, model):
        self._m = model

    def __getattr__(self, name):
        return getattr(self._m, name)

    def _backward_distortion(self, ctx, dy, accumulate):
        return None


def test_default_model_is_unchanged():
    from neural_imaging_amd.models import jpeg
    j = jpeg.JPEG(80, 'soft', device='cpu')
    assert j.entropy_weight is None
    assert repr(j) == 'JPEG(quality=80,codec="soft",trainable=False)'
    assert j.summary() == 'JPEG (soft) QF=80' and j.summary_compact() == 'JPEG (soft) QF=80'
    assert repr(jpeg.JPEG(70, 'soft', trainable=True, device='cpu')) == 'JPEG(quality=70,codec="soft",trainable=True)'
    assert repr(jpeg.JPEG(80, 'libjpeg', device='cpu')) == 'JPEG(quality=80,codec="libjpeg")'
    assert repr(jpeg.JPEG(50, 'soft', device='cpu', subsampling='4:2:0')) == \
        'JPEG(quality=50,codec="soft",trainable=False,subsampling="4:2:0")'
    assert repr(jpeg.JPEG(80, 'soft', device='cpu', entropy_weight=None)) == repr(j)
    with pytest.raises(NotImplementedError):
        jpeg.JPEG(70, 'libjpeg', device='cpu').backward({}, torch.zeros(1, 16, 16, 3))


def test_workflow_passes_the_weight_on_and_the_default_stays():
    from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification, _LazySum
    dist = {'downsampling': 'none', 'compression': 'jpeg', 'compression_params': {'quality': 50, 'codec': 'sin'}}
    wf = ManipulationClassification('UNet', distribution=dist, trainable={'nip'}, raw_patch_size=32, device='cpu')
    assert wf.codec.entropy_weight is None and 'JPEG (sin) QF=50' in wf.summary() and 'H+' not in wf.summary()
    assert repr(wf.codec) == 'JPEG(quality=50,codec="sin",trainable=False)'
    params = dict(dist['compression_params'], trainable=True, entropy_weight=0.5)
    wr = ManipulationClassification('UNet', distribution=dict(dist, compression_params=params), trainable={'nip', 'dcn'},
                                    raw_patch_size=32, device='cpu')
    assert wr.codec.entropy_weight == 0.5 and wr.is_trainable('dcn') and ' H+0.5' in wr.summary()
    assert wr._jpeg_manip.entropy_weight is None                  # no rate term on the shared 'jpeg' manipulation codec
    with pytest.raises(ValueError):
        ManipulationClassification('UNet', distribution=dict(dist, compression_params=dict(params, codec='libjpeg', trainable=False)),
                                   raw_patch_size=32, device='cpu')
    # the lazily read codec term: wa * a + w * b, and a + w * b as before
    a, b = torch.tensor([3.0]), torch.tensor([0.5])
    assert float(_LazySum(a, b, 4.0)) == 5.0 and float(_LazySum(a, b, 4.0, 2.0)) == 8.0


def test_abi_error_codes_before_any_launch():
    from neural_imaging_amd import _lib
    lib = _lib.load()
    assert lib.nimg_djpeg_entropy_workspace_bytes(0, 8, 8) == 0 and lib.nimg_djpeg_entropy_workspace_bytes(1, 0, 8) == 0
    one = lib.nimg_djpeg_entropy_workspace_bytes(1, 8, 8)
    assert one >= 512 * 8 * 2 and one % 16 == 0
    # the partial histograms stop growing with the batch (a wave walks several strips) and never shrink
    sizes = [lib.nimg_djpeg_entropy_workspace_bytes(n, 256, 256) for n in (1, 8, 64, 320, 640)]
    assert sizes == sorted(sizes) and sizes[-1] == sizes[-2] and sizes[-1] < (8 << 20)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)              # never dereferenced: every call below returns before a launch
    fwd, bwd = lib.nimg_djpeg_entropy_fwd, lib.nimg_djpeg_entropy_bwd
    big = 1 << 30
    assert fwd(None, None, 0, 8, 8, 1, None, None, 0, None) == 0                       # n == 0: a no-op
    assert bwd(None, None, 0, 8, 8, 1, 1.0, None, 0, None, 0, None, 0, None) == 0
    for h, w in ((12, 8), (8, 12), (0, 8), (8, -8)):
        assert fwd(p, p, 1, h, w, 1, p, p, big, None) == ERR_ARG
        assert bwd(p, p, 1, h, w, 1, 1.0, p, 0, None, 0, p, big, None) == ERR_ARG
    assert fwd(p, p, -1, 8, 8, 1, p, p, big, None) == ERR_ARG
    for rounding in (-1, 5):
        assert fwd(p, p, 1, 8, 8, rounding, p, p, big, None) == ERR_ARG
        assert bwd(p, p, 1, 8, 8, rounding, 1.0, p, 0, None, 0, p, big, None) == ERR_ARG
    for k in range(4):                     # x, qtab, entropy, workspace
        args = [p, p, 1, 8, 8, 1, p, p, big, None]
        args[(0, 1, 6, 7)[k]] = None
        assert fwd(*args) == ERR_ARG
    for k in range(4):                     # x, qtab, gx, workspace (dq may be null)
        args = [p, p, 1, 8, 8, 1, 1.0, p, 0, None, 0, p, big, None]
        args[(0, 1, 7, 11)[k]] = None
        assert bwd(*args) == ERR_ARG
    assert fwd(p, p, 1, 8, 8, 1, p, p, one - 1, None) == ERR_WORKSPACE
    assert bwd(p, p, 1, 8, 8, 1, 1.0, p, 0, None, 0, p, one - 1, None) == ERR_WORKSPACE
    assert bwd(p, p, 1, 8, 8, 1, 1.0, p, 0, p, 0, p, 0, None) == ERR_WORKSPACE


def test_five_centre_window_equals_the_full_sum():
    """Inside [-255.5, 256.5] a centre 2.5 or more away weighs < 2e-33 of the nearest (latent.hip, above t_weight): the five-centre
    sums equal the 512-centre sums to 1e-15 relative.  Grid: every half-integer and integer of the range, both ends, their float32
    neighbours inside, and a fine sweep; outside the range the restatement (and the kernel) takes the full loop."""
    half = np.arange(-511, 514) / 2.0                                      # -255.5 .. 256.5 in steps of 1/2
    ends = np.array([R.LO, R.HI, np.nextafter(np.float32(R.LO), np.float32(0)), np.nextafter(np.float32(R.HI), np.float32(0))], np.float64)
    sweep = np.linspace(R.LO, R.HI, 20001)
    near = np.concatenate([half + d for d in (-1e-3, 1e-3, -1e-7, 1e-7)])
    u = np.concatenate([half, ends, sweep, near[(near >= R.LO) & (near <= R.HI)]])
    assert u.min() == R.LO and u.max() == R.HI
    worst_S = worst_w = 0.0
    for part in np.array_split(u, 16):
        wfull = R.weight(part, R.CODEBOOK)
        S512 = wfull.sum(axis=1)
        k0 = np.clip(np.rint(part).astype(np.int64) + 255, 0, 511)
        S5 = np.zeros_like(S512)
        for j in range(-2, 3):
            k = k0 + j
            ok = (k >= 0) & (k <= 511)
            S5 += np.where(ok, wfull[np.arange(part.size), np.clip(k, 0, 511)], 0.0)
        worst_S = max(worst_S, float(np.abs(S5 / S512 - 1.0).max()))
        worst_w = max(worst_w, float(np.abs(R.window_weights(part) - R.full_weights(part)).max()))
    print('window: sums differ by {:.2e} relative, normalised weights by {:.2e}'.format(worst_S, worst_w))
    assert worst_S <= 1e-15 and worst_w <= 1e-15
    # the bound itself, at its worst point (a half-integer: the nearest centre 0.5 away, the first one left out 2.5 away)
    ratio = ((1.0 + (R.GAMMA * 2.5) ** 2 / R.V) / (1.0 + (R.GAMMA * 0.5) ** 2 / R.V)) ** (-(R.V + 1.0) / 2.0)
    assert ratio < 2e-33
    # outside the range: the full loop, bit for bit
    out = np.array([-255.5 - 1e-3, 256.5 + 1e-3, -400.0, 399.7, 1016.0, -1016.0])
    assert np.array_equal(R.window_weights(out), R.full_weights(out))
    # far outside, every weight is eps: the histogram term is uniform
    assert np.allclose(R.full_weights(np.array([1016.0])), 1.0 / 512, rtol=1e-12, atol=0)
