"""
Host checks of the sub-sampled differentiable JPEG: its float64 restatement (tests/djpeg_sub_ref.py) against
the reference's model at 4:4:4, its triangle filter against libjpeg's integer rule, how close it stands to the real codec
(tests/jpeg_ref.py - libjpeg restated), and the model / workflow surface.  No GPU.
"""
import numpy as np
import pytest
import torch

import djpeg_sub_ref as R
import jpeg_ref
from oracle import djpeg as odj
from oracle import tables as ot
from util import natural_images, to64

SUB = {'4:2:2': (2, 1), '4:2:0': (2, 2)}


def libjpeg_tables(quality):
    return to64(np.stack([jpeg_ref.qtable(quality, c).reshape(8, 8) for c in (0, 1, 1)]))


@pytest.mark.parametrize('mode', ['soft', 'sin', 'harmonic', 'identity', 'round'])
def test_restatement_is_the_reference_model_at_444(mode):
    x = natural_images(2, 16, 24, seed=3)
    rng = np.random.default_rng(4)
    gy = to64(rng.uniform(-1, 1, x.shape))
    tabs = [to64(ot.jpeg_qtable(60, c) * rng.uniform(0.7, 1.3, (8, 8))) for c in (0, 1)]
    grads = []
    for fn in ('ref', 'sub'):
        tl, tc = (t.clone().requires_grad_(True) for t in tabs)
        xt = to64(x).requires_grad_(True)
        q = torch.stack([tl, tc, tc])
        if fn == 'ref':
            y, xd, idx = odj.djpeg_torch(xt, mode=mode, q=q)
        else:
            y, (xl, xc), (il, ic), _ = R.djpeg_sub_torch(xt, q, mode, 1, 1)
            xd, idx = torch.cat([xl[:, None], xc], 1), torch.cat([il[:, None], ic], 1)
        (y * gy).sum().backward()
        grads.append((y.detach(), xd.detach(), idx.detach(), xt.grad, tl.grad, tc.grad))
    for a, b in zip(*grads):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize('sub', ['4:2:2', '4:2:0'])
def test_triangle_filter_against_the_integer_rule_and_its_adjoint(sub):
    hs, vs = SUB[sub]
    rng = np.random.default_rng(7)
    p = rng.integers(0, 256, (12, 20))
    p[:, :3] = 255 * (rng.random((12, 3)) > 0.5)                        # hard edges at the border
    up = R.upsample(to64(p)[None], hs, vs)[0].numpy()
    ref = jpeg_ref._upsample(p, hs, vs, 12, 20)
    assert up.shape == ref.shape == (12 * vs, 20 * hs)
    assert np.abs(up - ref).max() <= 1.0                                # the integer rule rounds once per pixel: within one level
    # the adjoint the backward kernel uses (a gather with clamped indices) is autograd's
    pt = to64(rng.normal(size=(2, 12, 20))).requires_grad_(True)
    g = to64(rng.normal(size=(2, 12 * vs, 20 * hs)))
    (R.upsample(pt, hs, vs) * g).sum().backward()
    adj = R.triangle_up_adjoint(g, 2)
    if vs == 2:
        adj = R.triangle_up_adjoint(adj, 1)
    assert float((adj - pt.grad).abs().max()) <= 1e-12


def test_mean_adjoint_and_index_override():
    x = to64(natural_images(1, 16, 32, seed=5))
    q = libjpeg_tables(75)
    y, _, (il, ic), _ = R.djpeg_sub_torch(x, q, 'round', 2, 2)
    y2, _, (il2, ic2), _ = R.djpeg_sub_torch(x, q, 'round', 2, 2, idx_override=(il, ic[:, 0], ic[:, 1]))
    assert torch.equal(y, y2) and torch.equal(il, il2) and torch.equal(ic, ic2)
    y3, _, _, _ = R.djpeg_sub_torch(x, q, 'round', 2, 2, idx_override=(il + 1, ic[:, 0], ic[:, 1]))
    assert not torch.equal(y, y3)
    p = to64(np.random.default_rng(1).normal(size=(1, 4, 8))).requires_grad_(True)
    R.box_down(p, 2, 2).sum().backward()
    assert torch.equal(p.grad, torch.full_like(p, 0.25))                # every pixel of a group receives g / (hs vs)


def real_decoded(x, quality, sub):
    hs, vs = jpeg_ref.SUBSAMPLING[sub]
    out = []
    for img in jpeg_ref.to_bytes(x):
        h, w, _ = img.shape
        out.append(jpeg_ref.to_float(jpeg_ref.decode_u8(jpeg_ref.coefficients(img, quality, hs, vs), h, w, quality, hs, vs)))
    return to64(np.stack(out))


@pytest.fixture(scope='module')
def psnr_table():
    """{(quality, sub): (sub model vs real sub, 4:4:4 model vs real sub, 4:4:4 model vs real 4:4:4)}: PSNR in dB over the batch."""
    x = natural_images(4, 64, 96)
    table = {}
    for quality in (50, 75, 90):
        q = libjpeg_tables(quality)
        m444 = R.djpeg_sub_torch(to64(x), q, 'round', 1, 1)[0]
        r444 = real_decoded(x, quality, '4:4:4')
        for sub, (hs, vs) in SUB.items():
            msub = R.djpeg_sub_torch(to64(x), q, 'round', hs, vs)[0]
            rsub = real_decoded(x, quality, sub)
            table[quality, sub] = (R.psnr(msub, rsub), R.psnr(m444, rsub), R.psnr(m444, r444))
    return table


@pytest.mark.parametrize('sub', ['4:2:2', '4:2:0'])
@pytest.mark.parametrize('quality', [50, 75, 90])
def test_sub_sampled_model_stands_next_to_the_real_codec(psnr_table, quality, sub):
    """The table of DESIGN.md 4j as a test: with box down-sampling and the triangle filter the float model (hard rounding, libjpeg's
    tables) is as close to a real sub-sampled file as the 4:4:4 model is to a real 4:4:4 file - at most 3 dB below that pair -
    and at least 8 dB closer to it than the 4:4:4 model.  PSNR over the batch natural_images(4, 64, 96) against the image
    tests/jpeg_ref.py decodes.  Measured: the gap is 11.3 dB at its smallest (QF 50, 4:2:2), the loss 2.8 dB at its largest (QF 75,
    4:2:0: 42.16 against 44.95 dB); at QF 90 the sub-sampled pair is 2.1 dB CLOSER than the 4:4:4 pair.  Image by image the gap is
    at least 10.3 dB and the loss at most 4.6 dB (one image at QF 75, 4:2:0)."""
    sub_real, m444_real, pair444 = psnr_table[quality, sub]
    print('QF {} {}: sub model {:.2f} dB, 4:4:4 model {:.2f} dB, 4:4:4 pair {:.2f} dB'.format(quality, sub, sub_real, m444_real, pair444))
    assert sub_real >= m444_real + 8.0, (sub_real, m444_real)
    assert sub_real >= pair444 - 3.0, (sub_real, pair444)


def test_model_surface():
    from neural_imaging_amd.models import jpeg
    with pytest.raises(ValueError):
        jpeg.JPEG(50, 'soft', subsampling='4:1:1')
    with pytest.raises(ValueError):
        jpeg.DifferentiableJPEG(50, 'soft', subsampling='4:1:1')
    # the default is today's model, string for string
    j = jpeg.JPEG(80, 'soft', device='cpu')
    assert j.subsampling == '4:4:4' and repr(j) == 'JPEG(quality=80,codec="soft",trainable=False)'
    assert j.summary() == 'JPEG (soft) QF=80' and j.summary_compact() == 'JPEG (soft) QF=80'
    assert repr(jpeg.JPEG(80, 'soft', device='cpu', subsampling='4:4:4')) == repr(j)
    assert repr(jpeg.JPEG(80, 'libjpeg', device='cpu')) == 'JPEG(quality=80,codec="libjpeg")'
    # a sub-sampling is appended
    s = jpeg.JPEG(50, 'soft', device='cpu', subsampling='4:2:0')
    assert s.summary() == 'JPEG (soft) QF=50 4:2:0' and s.summary_compact() == 'JPEG (soft) QF=50 4:2:0'
    assert repr(s) == 'JPEG(quality=50,codec="soft",trainable=False,subsampling="4:2:0")'
    assert jpeg.JPEG((50, 90), 'sin', device='cpu', subsampling='4:2:2').summary() == 'JPEG (sin) QF~[50,90] 4:2:2'
    assert repr(jpeg.JPEG(70, 'libjpeg', device='cpu', subsampling='4:2:2')) == 'JPEG(quality=70,codec="libjpeg",subsampling="4:2:2")'
    t = jpeg.JPEG(70, 'soft', trainable=True, device='cpu', subsampling='4:2:0')
    assert t.count_parameters() == 128 and t.summary().endswith(' 4:2:0') and t.summary().startswith('JPEG (soft) trainable QF~')
    # the refusals of the real codec stay
    with pytest.raises(NotImplementedError):
        jpeg.JPEG(70, 'libjpeg', device='cpu', subsampling='4:2:0').forward(torch.zeros(1, 16, 16, 3), training=True)
    with pytest.raises(NotImplementedError):
        jpeg.JPEG(70, 'libjpeg', device='cpu', subsampling='4:2:0').backward({}, torch.zeros(1, 16, 16, 3))


def test_ops_refuse_bad_factors_and_ragged_images_before_any_launch():
    from neural_imaging_amd import ops
    x = torch.zeros(1, 16, 16, 3)
    for hs, vs in ((1, 1), (1, 2), (4, 1)):
        with pytest.raises(ValueError):
            ops._djpeg_sub_shape(x, hs, vs)
    with pytest.raises(ValueError):
        ops._djpeg_sub_shape(torch.zeros(1, 24, 16, 3), 2, 2)            # 24 rows: one and a half MCUs at 4:2:0
    with pytest.raises(ValueError):
        ops._djpeg_sub_shape(torch.zeros(1, 16, 24, 3), 2, 1)
    assert ops._djpeg_sub_shape(torch.zeros(2, 24, 32, 3), 2, 1) == (2, 24, 32)


def test_workflow_accepts_and_reports_the_sub_sampling():
    from neural_imaging_amd.workflows.manipulation_classification import ManipulationClassification
    dist = {'downsampling': 'none', 'compression': 'jpeg',
            'compression_params': {'quality': 50, 'codec': 'soft', 'subsampling': '4:2:0'}}
    wf = ManipulationClassification('UNet', distribution=dist, trainable={'nip'}, raw_patch_size=32, device='cpu')
    assert wf.codec.subsampling == '4:2:0' and wf._jpeg_manip.subsampling == '4:4:4'     # the 'jpeg' manipulation stays 4:4:4
    assert 'JPEG (soft) QF=50 4:2:0' in wf.summary() and 'JPEG (soft) QF=50 4:2:0' in wf.summary_compact()
    wt = ManipulationClassification('UNet', distribution=dict(dist, compression_params=dict(
        dist['compression_params'], trainable=True)), trainable={'nip', 'dcn'}, raw_patch_size=32, device='cpu')
    assert wt.is_trainable('dcn') and wt.codec.count_parameters() == 128 and wt.codec.subsampling == '4:2:0'
    with pytest.raises(ValueError):
        ManipulationClassification('UNet', distribution=dict(dist, compression_params={'quality': 50, 'subsampling': '4:1:1'}),
                                   raw_patch_size=32, device='cpu')
