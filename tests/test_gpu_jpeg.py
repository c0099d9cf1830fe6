"""The baseline JPEG codec on the GPU (csrc/jpegc.hip through ops.jpeg_*, compression.jpeg_helpers and models.jpeg.JPEG with
codec='libjpeg'): coefficients, entropy-coded bytes, whole files and decoded images against the plain numpy restatement
(tests/jpeg_ref.py) and Pillow's golden files - everything exact, nothing has a tolerance."""
import numpy as np
import pytest
import torch

import jpeg_cases as cases
import jpeg_ref as ref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    return torch.device('cuda', 0)


def _guarded(size, fill, dev):
    """(tensor of size + GUARD bytes filled with `fill`, its first `size` bytes)."""
    t = torch.full((size + GUARD,), fill, dtype=torch.uint8, device=dev)
    return t, t[:size]


def _run(x, quality, subsampling, dev, capacity=None):
    """x uint8 / float32 numpy (n,h,w,3) -> (coefficients (n, blocks * 64), [segment bytes], lengths, decoded float32), with guard
    bytes behind the workspace and behind the output checked."""
    hs, vs = ops.jpeg_subsampling(subsampling)
    n, h, w, _ = x.shape
    from neural_imaging_amd import _lib
    ws_all, ws = _guarded(int(_lib.load().nimg_jpeg_workspace_bytes(n, h, w, hs, vs)), 0xa5, dev)
    xd = torch.from_numpy(np.array(x)).to(dev)                  # a copy: the case builders hand out read-only arrays
    coef = ops.jpeg_transform(xd, quality, hs, vs, workspace=ws)
    bound = n * ops.jpeg_ecd_bound(h, w, hs, vs)
    out_all, out = _guarded(bound if capacity is None else capacity, 0x5a, dev)
    data, lengths = ops.jpeg_encode(coef, h, w, hs, vs, out=out, workspace=ws)
    y = ops.jpeg_reconstruct(coef, h, w, quality, hs, vs, workspace=ws)
    lengths = lengths.cpu().numpy().astype(np.int64)
    blob = data.cpu().numpy()
    total = int(lengths.sum())
    assert (ws_all[-GUARD:] == 0xa5).all(), 'a write behind the workspace'
    assert (out_all[-GUARD:] == 0x5a).all(), 'a write behind the output'
    assert (blob[min(total, len(blob)):] == 0x5a).all(), 'a write behind the last segment'
    ends = np.concatenate([[0], np.cumsum(lengths)])
    segments = [blob[ends[i]:ends[i + 1]].tobytes() for i in range(n)]
    return coef.cpu().numpy().reshape(n, -1), segments, lengths, y.cpu().numpy()


@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_every_stage_equals_the_restatement(dev, case):
    x, r = cases.build(case), cases.reference(case)
    coef, segments, lengths, y = _run(x, case.quality, case.subsampling, dev)
    assert np.array_equal(coef, r.flat), 'coefficients'
    assert lengths.tolist() == [len(e) for e in r.ecds], 'lengths'
    assert segments == r.ecds, 'entropy-coded bytes'
    assert np.array_equal(y.view(np.uint32), ref.to_float(r.decoded).view(np.uint32)), 'decoded image'
    files = jh.encode_batch(x, case.quality, case.subsampling)
    assert files == r.files
    if case.golden:
        gx, gfiles, grgb = cases.golden()[case.name]
        assert files == gfiles, 'not the file libjpeg writes'
        assert np.array_equal(y.view(np.uint32), ref.to_float(grgb).view(np.uint32)), 'not the image libjpeg decodes'


@pytest.mark.parametrize('name', ['noise+smooth+constant+checker_16x24_q75_422', 'smooth+noise+half_13x21_q95_420',
                                  'noise+mixed_128x192_q30_420'])
def test_image_in_a_batch_equals_image_alone(dev, name):
    case = cases.by_name(name)
    x = cases.build(case)
    _, together, _, y = _run(x, case.quality, case.subsampling, dev)
    for i in range(len(x)):
        _, alone, _, yi = _run(x[i:i + 1], case.quality, case.subsampling, dev)
        assert alone[0] == together[i] and np.array_equal(yi[0], y[i])
    assert len({len(s) for s in together}) == len(together)           # the lengths differ


def test_nothing_is_written_beyond_the_capacity(dev, monkeypatch):
    case = cases.by_name('noise+smooth+constant+checker_16x24_q75_422')
    x, r = cases.build(case), cases.reference(case)
    want = b''.join(r.ecds)
    for short in (1, 2, len(r.ecds[-1]) + 3, len(want) - 8):
        _, segments, lengths, _ = _run(x, case.quality, case.subsampling, dev, capacity=len(want) - short)
        assert lengths.tolist() == [len(e) for e in r.ecds]                      # the lengths still say what is needed
        assert b''.join(segments) == want[:len(want) - short]
    # ... and a batch that was given too little is coded again with what its lengths ask for
    monkeypatch.setattr(ops, 'jpeg_ecd_bound', lambda *a: 16)
    assert jh.encode_batch(x, case.quality, case.subsampling) == r.files


def test_float_input_goes_through_the_reference_conversion(dev):
    """(255 * x).astype(uint8) in float32, after x / 255 when the batch's maximum exceeds 1: all 256 byte values either way, values
    between bytes (truncated) and beyond them (clamped)."""
    k = np.arange(256, dtype=np.float32)
    for values in (k, k / np.float32(255), np.array([-0.5, 0.0, 0.9999, 0.5, 1.0, 0.00392], np.float32),
                   np.array([-3.0, 254.9, 300.0, 1.0001, 77.5], np.float32)):
        x = np.resize(values, (1, 16, 24, 3)).astype(np.float32)
        x[0, 1:] = x[0, 1:][:, ::-1]
        byte = ref.to_bytes(x)
        if values is k or values.max() <= 1:
            assert np.array_equal(byte, (255 * (x / 255 if x.max() > 1 else x)).clip(0, 255).astype(np.uint8))
        a = _run(x, 100, '4:2:0', dev)[0]
        b = _run(byte, 100, '4:2:0', dev)[0]
        assert np.array_equal(a, b) and np.array_equal(b[0], ref.flat_coefficients(ref.coefficients(byte[0], 100, 2, 2)))


def test_compress_batch(dev):
    case = cases.by_name('smooth+noise+half_13x21_q95_420')
    x, r = cases.build(case), cases.reference(case)
    sizes = [len(f) for f in r.files]
    for batch in (x, x.astype(np.float32), x.astype(np.float32) / np.float32(255)):
        # uint8 input is converted like any other (x / 255, 255 x, truncated), which is the identity on whole bytes
        y, b = jh.compress_batch(batch, case.quality, subsampling=case.subsampling)
        assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == x.shape and isinstance(b, list)
        assert b == sizes and np.array_equal(y, ref.to_float(r.decoded))
        _, b = jh.compress_batch(batch, case.quality, effective=True, subsampling=case.subsampling)
        assert b == [s - 177 for s in sizes]
        y, b = jh.compress_batch(batch[1], case.quality, subsampling=case.subsampling)
        assert y.dtype == np.float64 and y.shape == x.shape[1:] and isinstance(b, int) and b == sizes[1]
        assert np.array_equal(y, r.decoded[1] / 255)
        assert jh.compress_batch(batch[1], case.quality, True, case.subsampling)[1] == sizes[1] - 177
    assert jh.JPEGMarkerStats(jh.encode_batch(x, case.quality, case.subsampling)[1]).get_effective_bytes() == sizes[1] - 177
    y, b = jh.compress_batch(x[:1], 30)                                            # defaults: 4:4:4
    assert b == [len(ref.compress(x[0], 30)[0])]
    for fn in (jh.compress_batch, jh.encode_batch):
        with pytest.raises(ValueError):
            fn(x, 75, subsampling='4:1:1')
    with pytest.raises(ValueError):
        jh.compress_batch(x, 0)


def _bisect(gap):
    """The reference's search (jpeg_helpers.py:55-79) over any deviation function."""
    low, high = 1, 95
    gl, gh = gap(low), gap(high)
    while high - low > 1:
        if gl * gh > 0:
            raise ValueError('same deviation')
        mid = (low + high) // 2
        gm = gap(mid)
        if gm * gh > 0:
            high, gh = mid, gm
        else:
            low, gl = mid, gm
    return low if abs(gh) > abs(gl) else high


@pytest.mark.parametrize('subsampling', ['4:4:4', '4:2:0'])
def test_match_quality_bpp(dev, subsampling):
    img = cases.build(cases.by_name('mixed_64x72_q1_444'))[0][:40, :48].astype(np.float32) / np.float32(255)
    byte = ref.to_bytes(img)
    for target in (3.5, 5.0):              # whole files: the 623 header bytes alone are 2.6 bpp of a 40 x 48 image
        expect = _bisect(lambda q: 8 * len(ref.encode(byte, q, subsampling)) / 40 / 48 - target)
        assert jh.match_quality(img, target, match='bpp', subsampling=subsampling) == expect
    with pytest.raises(ValueError, match='Same deviation'):
        jh.match_quality(img, 100.0, match='bpp')
    with pytest.raises(ValueError, match='Invalid argument'):
        jh.match_quality(img, 1.0, match='psnr')


def test_match_quality_ssim(dev):
    from neural_imaging_amd.helpers import metrics
    img = cases.build(cases.by_name('mixed_64x72_q1_444'))[0][:40, :48].astype(np.float32) / np.float32(255)
    target = 0.9
    q = jh.match_quality(img, target)
    assert 1 <= q <= 95

    def gap(k):
        return metrics.ssim(img, jh.compress_batch(img, k)[0]) - target

    far = q - 1 if gap(q) < 0 else q + 1                      # the neighbour away from the target
    assert 1 <= far <= 95 and abs(gap(far)) >= abs(gap(q))
    with pytest.raises(ValueError, match='Same deviation'):
        jh.match_quality(img, 2.0)


def test_jpeg_model_libjpeg_codec(dev):
    from neural_imaging_amd.device import DeviceArray
    from neural_imaging_amd.models.jpeg import JPEG
    from neural_imaging_amd.training.validation import validate_jpeg
    case = cases.by_name('mixed+smooth_128x192_q75_444')
    x = cases.build(case)[:, :32, :48].astype(np.float32) / np.float32(255)
    codec, soft = JPEG(75, codec='libjpeg', device=dev), JPEG(75, codec='soft', device=dev)
    y = codec.process(x)
    assert isinstance(y, DeviceArray) and np.array_equal(y.numpy(), jh.compress_batch(x, 75)[0])
    y, entropy = codec.process(x, 40, return_entropy=True)
    assert np.isnan(entropy) and np.array_equal(y.numpy(), jh.compress_batch(x, 40)[0])
    for quality in ((30, 90), (10, 35, 60, 85)):              # a range / a set: drawn from numpy's RNG exactly as the other codecs draw
        np.random.seed(7)
        y = codec.process(x, quality)
        state = np.random.get_state()[1].copy()
        np.random.seed(7)
        drawn = JPEG.resolve_quality(quality)
        assert np.array_equal(y.numpy(), jh.compress_batch(x, drawn)[0])
        np.random.seed(7)
        soft.process(x, quality)
        assert np.array_equal(np.random.get_state()[1], state)
    with pytest.raises(ValueError):
        JPEG(None, codec='libjpeg', device=dev).process(x)
    xd = torch.from_numpy(x).to(dev)
    assert np.array_equal(codec.forward(xd)[0].cpu().numpy(), jh.compress_batch(x, 75)[0]) and codec.forward(xd)[1] is None
    with pytest.raises(NotImplementedError):
        codec.forward(xd, training=True)
    with pytest.raises(NotImplementedError):
        codec.backward({}, xd)
    assert repr(codec) == 'JPEG(quality=75,codec="libjpeg")'

    class Data(object):
        count_validation = 2

        def next_validation_batch(self, b, batch_size):
            return x[b * batch_size:(b + 1) * batch_size]

    res = validate_jpeg(codec, Data(), batch_size=1)
    from neural_imaging_amd.helpers import metrics
    decoded = jh.compress_batch(x, 75)[0]
    assert np.isnan(res['entropy']) and abs(res['ssim'] - float(np.mean(metrics.ssim(x, decoded)))) < 1e-6
    assert abs(res['psnr'] - float(np.mean(metrics.psnr(x, decoded)))) < 1e-3
