"""Rate-distortion on the device: the per-item JPEG kernels (csrc/jpegc_items.hip through ops.jpeg_*_items),
jpeg_helpers.rate_distortion / match_quality_batch, the MS-SSIM metric (csrc/msssim.hip through ops.msssim, helpers.metrics) and the
tables of compression.ratedistortion.  The codec side is exact - every item equals the single-quality path and the numpy restatement
(tests/jpeg_ref.py) byte for byte; MS-SSIM is held to the float64 oracle with the bound of the MS-SSIM loss."""
import json
import os

import numpy as np
import pytest
import torch

import glue_cases
import jpeg_ref as ref
import ratedist_cases as cases
from neural_imaging_amd import ops
from neural_imaging_amd.compression import codec, jpeg_helpers as jh, ratedistortion as rd
from neural_imaging_amd.helpers import metrics

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    return torch.device('cuda', 0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _segments(data, lengths):
    lengths = lengths.cpu().numpy().astype(np.int64)
    blob = data.cpu().numpy()
    ends = np.concatenate([[0], np.cumsum(lengths)])
    return [blob[ends[i]:ends[i + 1]].tobytes() for i in range(len(lengths))], lengths


# ---- 1. items against the single-quality entry points and the restatement ---------------------------------------------------
@pytest.mark.parametrize('case', cases.ITEM_CASES, ids=cases.ITEM_IDS)
@pytest.mark.parametrize('kind', ['uint8', 'float32'])
def test_every_item_equals_its_image_alone_at_its_quality(dev, case, kind):
    from neural_imaging_amd import _lib
    hs, vs = ops.jpeg_subsampling(case.subsampling)
    h, w, n_items = case.h, case.w, case.n_items
    x8 = cases.sources(case)
    host = np.array(x8) if kind == 'uint8' else x8.astype(np.float32) / np.float32(255)
    x = torch.from_numpy(host).to(dev)
    q = cases.qualities(case)
    size = int(_lib.load().nimg_jpeg_workspace_bytes(n_items, h, w, hs, vs))
    ws_all = torch.full((size + GUARD,), 0xa5, dtype=torch.uint8, device=dev)
    ws = ws_all[:size]
    coef, err = ops.jpeg_transform_items(x, q, hs, vs, workspace=ws)
    data, lengths = ops.jpeg_encode(coef, h, w, hs, vs, workspace=ws)
    y, err2 = ops.jpeg_reconstruct_items(coef, h, w, q, hs, vs, workspace=ws)
    _, counted = ops.jpeg_encode(coef, h, w, hs, vs, workspace=ws, capacity=1)          # the byte counts alone, as rate_distortion asks
    assert int(err.item()) == 0 and int(err2.item()) == 0
    assert (ws_all[-GUARD:] == 0xa5).all(), 'a write behind the workspace'
    assert tuple(coef.shape) == (n_items, ops.jpeg_geometry(h, w, hs, vs)[0], 64) and tuple(y.shape) == (n_items, h, w, 3)
    segments, lengths = _segments(data, lengths)
    assert np.array_equal(counted.cpu().numpy(), lengths)
    coef, y = coef.cpu().numpy(), y.cpu().numpy()
    for j in range(n_items):
        src = j % case.n_src
        one = x[src:src + 1]
        c1 = ops.jpeg_transform(one, q[j], hs, vs)
        d1, l1 = ops.jpeg_encode(c1, h, w, hs, vs)
        y1 = ops.jpeg_reconstruct(c1, h, w, q[j], hs, vs)
        s1, l1 = _segments(d1, l1)
        what = 'item {} (image {}, quality {})'.format(j, src, q[j])
        assert np.array_equal(coef[j], c1.cpu().numpy()[0]), what + ': coefficients'
        assert lengths[j] == l1[0] and segments[j] == s1[0], what + ': entropy-coded segment'
        assert np.array_equal(_bits(y[j]), _bits(y1.cpu().numpy()[0])), what + ': decoded image'
        r = cases.restated(case, src, q[j])
        assert np.array_equal(coef[j].reshape(-1), r.flat.reshape(-1)), what + ': coefficients of the restatement'
        assert segments[j] == r.ecd and jh.jpeg_header(h, w, q[j], case.subsampling) + segments[j] + b'\xff\xd9' == r.file, what
        assert np.array_equal(_bits(y[j]), _bits(r.decoded)), what + ': the image the restatement decodes'


def test_one_above_one_flag_per_call(dev):
    """Float input is divided by 255 when ANY value of the call's source images exceeds 1 - one flag, whatever the items' qualities."""
    case = cases.ITEM_CASES[0]
    x8 = cases.sources(case)
    x = x8.astype(np.float32) / np.float32(255)
    x[1] = x8[1].astype(np.float32)                                   # one source image in 0..255: every image is divided
    q = [30, 75, 49]
    coef, _ = ops.jpeg_transform_items(torch.from_numpy(x).to(dev), q, 2, 2)
    divided = ref.to_bytes(x)                                         # x / 255 for all three, then (255 x) truncated
    assert not np.array_equal(divided[0], x8[0]) and np.abs(divided[1].astype(int) - x8[1]).max() <= 1
    for j in range(3):
        want = ops.jpeg_transform(torch.from_numpy(divided[j:j + 1]).to(dev), q[j], 2, 2)
        assert np.array_equal(coef.cpu().numpy()[j], want.cpu().numpy()[0]), j


# ---- 4. a quality byte outside 1..100 ------------------------------------------------------------------------------------------
def test_out_of_range_quality_is_clamped_and_flagged(dev):
    """Past the Python check, straight to the ABI: the kernels read the tables of quality 1 / 100 instead and raise the flag."""
    case = cases.ITEM_CASES[0]
    hs, vs = ops.jpeg_subsampling(case.subsampling)
    x = torch.from_numpy(np.array(cases.sources(case))).to(dev)
    with pytest.raises(ValueError):
        ops.jpeg_transform_items(x, [0, 50, 75], hs, vs)              # on the host the values are seen and refused
    with pytest.raises(ValueError):
        ops.jpeg_transform_items(x, [50, 101, 75], hs, vs)
    bad = torch.tensor([0, 101, 50], dtype=torch.uint8, device=dev)
    good = [1, 100, 50]
    coef, err = ops.jpeg_transform_items(x, bad, hs, vs)
    want, err0 = ops.jpeg_transform_items(x, good, hs, vs)
    assert int(err.item()) != 0 and int(err0.item()) == 0
    assert torch.equal(coef, want)
    y, err = ops.jpeg_reconstruct_items(want, case.h, case.w, bad, hs, vs)
    y0, err0 = ops.jpeg_reconstruct_items(want, case.h, case.w, good, hs, vs)
    assert int(err.item()) != 0 and int(err0.item()) == 0
    assert torch.equal(y, y0)
    only = torch.tensor([75, 75, 255], dtype=torch.uint8, device=dev)          # the flag of a single offender in the last item
    assert int(ops.jpeg_transform_items(x, only, hs, vs)[1].item()) != 0


# ---- 2. rate_distortion against the loop it replaces ------------------------------------------------------------------------------
RD_QUALITIES = (95, 49, 30, 10)


@pytest.mark.parametrize('subsampling', ['4:2:0', '4:4:4'])
def test_rate_distortion_equals_the_loop(dev, subsampling):
    x = cases.rd_images(176, 192)
    out, images = jh.rate_distortion(x, RD_QUALITIES, subsampling=subsampling, effective=True, want_images=True)
    plain = jh.rate_distortion(x, RD_QUALITIES, subsampling=subsampling, effective=False)
    assert tuple(images.shape) == (4, 3, 176, 192, 3) and images.is_cuda
    assert set(out) == set(plain) == {'ssim', 'psnr', 'msssim', 'msssim_db', 'bytes', 'bpp'}
    images = images.cpu().numpy()
    for k, quality in enumerate(RD_QUALITIES):
        y, sizes = jh.compress_batch(x, quality, effective=True, subsampling=subsampling)
        assert out['bytes'][k].tolist() == sizes
        assert plain['bytes'][k].tolist() == jh.compress_batch(x, quality, effective=False, subsampling=subsampling)[1]
        assert np.array_equal(_bits(images[k]), _bits(y)), 'decoded images at quality {}'.format(quality)
        assert np.array_equal(out['ssim'][k], metrics.ssim(x, y)) and np.array_equal(out['psnr'][k], metrics.psnr(x, y))
        assert np.array_equal(out['msssim'][k], metrics.msssim(x, y)) and np.array_equal(out['msssim_db'][k], metrics.msssim_db(x, y))
    for t in (out, plain):
        assert t['bytes'].shape == (4, 3) and np.array_equal(t['bpp'], 8 * t['bytes'] / 176 / 192)
        assert np.isfinite(t['msssim']).all() and (t['msssim'] > 0.3).all() and (t['msssim'] < 1).all()
    assert np.array_equal(out['ssim'], plain['ssim']) and (out['bytes'] < plain['bytes']).all()


def test_rate_distortion_in_groups_of_qualities(dev, monkeypatch):
    """A workspace budget that holds one quality at a time: the same table from four item calls."""
    x = cases.rd_images(176, 192)
    whole = jh.rate_distortion(x, RD_QUALITIES, subsampling='4:2:0')
    calls = []
    real = ops.jpeg_transform_items
    monkeypatch.setattr(ops, 'jpeg_transform_items', lambda *a, **k: calls.append(1) or real(*a, **k))
    assert all(np.array_equal(whole[k], v, equal_nan=True) for k, v in jh.rate_distortion(x, RD_QUALITIES, subsampling='4:2:0').items())
    assert len(calls) == 1
    monkeypatch.setattr(jh, 'RD_WORKSPACE_BUDGET', int(ops._lib.load().nimg_jpeg_workspace_bytes(3, 176, 192, 2, 2)))
    parts = jh.rate_distortion(x, RD_QUALITIES, subsampling='4:2:0')
    assert len(calls) == 1 + len(RD_QUALITIES)
    assert all(np.array_equal(whole[k], parts[k]) for k in whole)


def test_rate_distortion_of_images_too_small_for_msssim(dev, monkeypatch):
    import warnings
    x = cases.rd_images(40, 56)
    monkeypatch.setattr(metrics, '_MSSSIM_WARNED', False)
    with pytest.warns(UserWarning, match='MS-SSIM'):
        out = jh.rate_distortion(x, RD_QUALITIES, subsampling='4:2:0')
    assert np.isnan(out['msssim']).all() and np.isnan(out['msssim_db']).all()
    for k, quality in enumerate(RD_QUALITIES):
        y, sizes = jh.compress_batch(x, quality, effective=True, subsampling='4:2:0')
        assert out['bytes'][k].tolist() == sizes and np.array_equal(out['ssim'][k], metrics.ssim(x, y))
        assert np.array_equal(out['psnr'][k], metrics.psnr(x, y))
    with warnings.catch_warnings():                                   # said once
        warnings.simplefilter('error')
        assert np.isnan(metrics.msssim(x, x)).all() and np.isnan(metrics.msssim(x[0], x[0])) and np.isnan(metrics.msssim_db(x[0], x[0]))


# ---- 3. match_quality_batch -------------------------------------------------------------------------------------------------
MATCH_AT = (15, 40, 65, 88)            # the targets are what the restatement gives at these qualities: the answers differ per image


SCALAR_TARGET = {'bpp': 2.1, 'ssim': 0.9}            # one target inside the range of all four images


def _restated_targets(x, match):
    """Per image: the bpp of the restatement's file, or the float64 SSIM of the image it decodes, at MATCH_AT - and the same at the
    end points 1 and 95, which have to bracket it, and SCALAR_TARGET, for the reference's bisection not to raise."""
    u8 = ref.to_bytes(x)

    def value(i, quality):
        data, decoded = ref.compress(u8[i], quality, '4:4:4')
        if match == 'bpp':
            return 8 * len(data) / x.shape[1] / x.shape[2]
        return float(glue_cases.ssim_ref(x[i:i + 1], ref.to_float(decoded)[None], 'skimage')[0])
    target = np.array([value(i, q) for i, q in enumerate(MATCH_AT)])
    for i in range(len(x)):
        lo, hi = value(i, 1), value(i, 95)
        assert lo < target[i] < hi and lo < SCALAR_TARGET[match] < hi, 'image {}: the end points do not bracket the target'.format(i)
    return target


@pytest.mark.parametrize('match', ['bpp', 'ssim'])
def test_match_quality_batch_equals_match_quality_per_image(dev, monkeypatch, match):
    x = cases.match_images()
    target = _restated_targets(x, match)
    want = [jh.match_quality(img, t, match) for img, t in zip(x, target)]
    assert len(set(want)) >= 3, want
    calls = []
    real = ops.jpeg_transform_items
    monkeypatch.setattr(ops, 'jpeg_transform_items', lambda *a, **k: calls.append(1) or real(*a, **k))
    got = jh.match_quality_batch(x, target, match)
    assert got.dtype.kind == 'i' and got.tolist() == want
    assert 0 < len(calls) <= 9
    n_calls = len(calls)
    del calls[:]
    assert jh.match_quality_batch(x[:2], target[:2], match).tolist() == want[:2] and len(calls) == n_calls       # whatever n is
    # a scalar target: the same for every image
    alone = [jh.match_quality(img, SCALAR_TARGET[match], match) for img in x]
    assert jh.match_quality_batch(x, SCALAR_TARGET[match], match).tolist() == alone and len(set(alone)) >= 3, alone
    # a target outside one image's range
    off = target.copy()
    off[2] = 0.01 if match == 'bpp' else 1.5
    with pytest.raises(ValueError, match='Same deviation for both end-points 1 - 95.*image 2'):
        jh.match_quality_batch(x, off, match)
    with pytest.raises(ValueError, match='Same deviation'):
        jh.match_quality(x[2], off[2], match)


# ---- 5. MS-SSIM against the float64 oracle ----------------------------------------------------------------------------------
def _loss_close(got, want):
    assert abs(got - want) <= 2e-6 * max(1.0, abs(want)), (got, want)          # (the bound of tests/test_gpu_glue_exact.py)


@pytest.fixture(scope='module')
def msssim_pairs():
    from oracle import tfops as T
    from util import to64
    y, t = glue_cases.image_pair(3, 176, 192, 3, 57)
    a = np.concatenate([y, t[:1], t[:1]])
    b = np.concatenate([t, t[:1], 1 - t[:1]]).astype(np.float32)
    want = T.ssim_multiscale(to64(a), to64(b), 1.0).numpy()
    assert want[3] == 1.0 and want[4] == 0.0 and (want[:3] > 0.5).all() and (want[:3] < 1).all()
    return a, b, want


def test_msssim_per_image(dev, msssim_pairs):
    a, b, want = msssim_pairs
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    got = ops.msssim(ad, bd)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5,)
    got = got.cpu().numpy()
    for i in range(5):
        print('image {}: 255 (1 - msssim) {!r} (oracle {!r})'.format(i, 255 * (1 - got[i]), 255 * (1 - want[i])))
    for i in range(5):
        _loss_close(255 * (1 - got[i]), 255 * (1 - want[i]))
    assert got[3] == 1.0 and got[4] == 0.0 and not np.isnan(got).any()
    for i in range(5):                                                  # alone = in the batch, bit for bit
        assert float(ops.msssim(ad[i:i + 1], bd[i:i + 1]).item()) == got[i]
    assert np.array_equal(ops.msssim(ad[1:4], bd[1:4]).cpu().numpy(), got[1:4])
    loss, _ = ops.msssim_loss(ad, bd)
    _loss_close(float(np.mean(255 * (1 - got))), float(loss.item()))
    assert np.array_equal(metrics.msssim(a, b), got) and metrics.msssim(a[0], b[0]) == got[0]
    with np.errstate(divide='ignore'):
        assert np.array_equal(metrics.msssim_db(a, b), -10 * np.log10(1 - got)) and np.isinf(metrics.msssim_db(a[3], b[3]))


def test_msssim_size_rule(dev):
    a = torch.zeros((1, 168, 176, 3), device=dev)
    with pytest.raises(ValueError):
        ops.msssim(a, a)
    with pytest.raises(ValueError):
        ops.msssim_loss(a, a)
    with pytest.raises(ValueError):
        ops.msssim(torch.zeros((1, 160, 192, 3), device=dev), torch.zeros((1, 160, 192, 3), device=dev))


# ---- 6. / 7. the tables -------------------------------------------------------------------------------------------------------
def test_get_jpeg_df(dev, tmp_path):
    import pandas as pd
    from PIL import Image
    x = cases.write_pngs(tmp_path)
    df = rd.get_jpeg_df(str(tmp_path), write_files=True)
    assert list(df.columns) == ['image_id', 'filename', 'codec', 'quality', 'ssim', 'psnr', 'msssim', 'msssim_db', 'bytes', 'bpp']
    qualities = list(range(95, 5, -5))
    assert len(df) == 54 and df['image_id'].tolist() == [i for i in range(3) for _ in qualities]
    assert df['quality'].tolist() == qualities * 3 and df['filename'].tolist() == [f for f in ('a.png', 'b.png', 'c.png') for _ in qualities]
    assert set(df['codec']) == {'jpeg'}
    want, images = jh.rate_distortion(x, qualities, effective=True, want_images=True)
    for col in ('ssim', 'psnr', 'msssim', 'msssim_db', 'bytes', 'bpp'):
        assert np.array_equal(df[col].to_numpy(dtype=np.float64).reshape(3, 18), want[col].T.astype(np.float64)), col
    assert np.isfinite(df['msssim'].to_numpy(dtype=np.float64)).all()
    back = pd.read_csv(os.path.join(str(tmp_path), 'jpeg.csv'), index_col=False, float_precision='round_trip')
    assert list(back.columns) == list(df.columns) and len(back) == 54
    for col in df.columns:
        if col in ('filename', 'codec'):
            assert back[col].tolist() == df[col].tolist()
        else:
            assert np.array_equal(back[col].to_numpy(dtype=np.float64), df[col].to_numpy(dtype=np.float64)), col
    again = rd.get_jpeg_df(str(tmp_path))                                # the cached file: the numbers that were computed
    assert again['bytes'].tolist() == df['bytes'].tolist() and again['ssim'].tolist() == df['ssim'].tolist()
    assert again['msssim_db'].tolist() == df['msssim_db'].tolist()
    images = images.cpu().numpy()
    for i, stem in enumerate('abc'):
        for k, quality in enumerate(qualities):
            with Image.open(os.path.join(str(tmp_path), stem, 'jpeg_q{:03d}.png'.format(quality))) as im:
                assert np.array_equal(np.asarray(im), (255 * images[k, i]).astype(np.uint8))
    whole = rd.get_jpeg_df(str(tmp_path), effective_bytes=False, force_calc=True)
    assert (whole['bytes'].to_numpy() - df['bytes'].to_numpy() == 177).all()


def _save_dcn(dcn, out, reference_layout):
    """A training directory as training.compression.train_dcn leaves it (progress.json + checkpoint + arguments), or with the
    reference's progress.json, whose model record sits under 'codec'."""
    os.makedirs(out)
    record = {'performance': dcn.performance, 'summary': {'Epoch': 0}, 'args': dcn.get_hyperparameters()}
    if reference_layout:
        record = {'codec': {'model': dcn.class_name, 'args': dcn.get_hyperparameters(), 'performance': dcn.performance}}
    with open(os.path.join(out, 'progress.json'), 'w') as f:
        json.dump(record, f, indent=4, default=lambda o: float(o))
    dcn.save_model(out, 0, save_args=not reference_layout, quiet=True)          # (next to the reference's log, a second JSON file
    # without a 'codec' record would be the one codec.restore reads whenever the directory lists it first)


def test_get_dcn_df(dev, tmp_path):
    from neural_imaging_amd.models import compression
    images = tmp_path / 'images'
    images.mkdir()
    x = cases.write_pngs(images)
    root = tmp_path / 'models'
    models = []
    # two directories as train_dcn leaves them, and a third with the reference's progress.json
    for k, (nf, layout) in enumerate(((4, False), (8, False), (12, True))):
        dcn = compression.TwitterDCN(patch_size=176, n_features=nf, device=dev, seed=5 + k)
        _save_dcn(dcn, str(root / 'run{}'.format(k) / dcn.scoped_name), layout)
        models.append(dcn)
    df = rd.get_dcn_df(str(images), str(root), write_files=True)
    assert list(df.columns) == ['image_id', 'filename', 'model_dir', 'codec', 'ssim', 'psnr', 'msssim', 'msssim_db', 'entropy', 'bytes',
                                'bpp', 'layers', 'quantization', 'entropy_reg', 'codebook', 'latent', 'latent_shape', 'n_features']
    assert len(df) == 9 and df['image_id'].tolist() == [0, 1, 2] * 3 and df['filename'].tolist() == ['a.png', 'b.png', 'c.png'] * 3
    assert df['n_features'].tolist() == [4] * 3 + [8] * 3 + [12] * 3
    assert df['model_dir'].tolist() == ['run0/'] * 3 + ['run1/'] * 3 + ['run2/'] * 3
    assert os.path.isfile(os.path.join(str(images), 'dcn-models.csv'))
    for k, dcn in enumerate(models):
        rows = df.iloc[3 * k:3 * k + 3]
        batch_y, stats = codec.compress_n_stats(x, dcn)
        for col in ('ssim', 'psnr', 'entropy', 'bpp'):
            assert np.array_equal(rows[col].to_numpy(dtype=np.float64), stats[col]), col
        assert rows['bytes'].tolist() == [len(codec.compress(x[i], dcn)) for i in range(3)]
        assert np.array_equal(rows['msssim'].to_numpy(dtype=np.float64), metrics.msssim(x, batch_y))
        assert set(rows['codec']) == {dcn.model_code} and set(rows['latent_shape']) == {'22x22x{}'.format(4 * (k + 1))}
        assert set(rows['latent']) == {22 * 22 * 4 * (k + 1)} and set(rows['codebook']) == {dcn._h.rounding}
        assert set(rows['quantization']) == {'{}-{:.0f}bpf'.format(dcn._h.rounding, dcn._h.latent_bpf)}
        assert os.path.isfile(os.path.join(str(images), 'a', dcn.model_code.replace('/', '-') + '.png'))
    again = rd.get_dcn_df(str(images), str(root))
    assert again['bytes'].tolist() == df['bytes'].tolist() and again['entropy'].tolist() == df['entropy'].tolist()
