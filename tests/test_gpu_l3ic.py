"""The l3ic bitstream on the GPU (neural_imaging_amd.compression.codec over nimg_l3ic_*): quantisation against
scipy.cluster.vq.vq, histograms / frequencies / payload bytes against the plain-Python restatement tests/l3ic_ref.py and the
golden streams, decoding in both directions, malformed streams, and the codec end to end on a seeded TwitterDCN."""
import os

import numpy as np
import pytest
import torch
from scipy.cluster.vq import vq

import l3ic_ref as ref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import codec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'l3ic_streams.npz')
UNIT = np.arange(-15, 17, dtype=np.float32)                                  # the DCN codebook at latent_bpf 5
UNEVEN = np.array([-7.0, -2.5, -2.0, -0.25, 0.0, 0.1, 1.0, 3.5, 12.0], np.float32)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    return torch.device('cuda', 0)


def _laplace(rng, n, k, scale=2.0):
    p = np.exp(-np.abs(np.arange(k) - (k - 1) / 2) / scale)
    return rng.choice(k, n, p=p / p.sum()).astype(np.uint8)


def _encode_layers(layers, dev):
    """GPU payloads of equally long index layers -> (list of bytes, hist, freq)."""
    idx = torch.from_numpy(np.stack(layers)).to(dev)
    data, lengths, hist, freq = ops.l3ic_encode(idx, want_stats=True)
    lengths = lengths.cpu().numpy().astype(np.int64)
    blob = data[:int(lengths.sum())].cpu().numpy().tobytes()
    ends = np.concatenate([[0], np.cumsum(lengths)])
    return [blob[ends[i]:ends[i + 1]] for i in range(len(layers))], hist.cpu().numpy(), freq.cpu().numpy()


def _decode_layers(payloads, n_sym, codebook, dev):
    """GPU decode of single-layer streams of a (1, 1, n_sym, 1) latent each (image i = payload i)."""
    h, w = (1, n_sym) if n_sym <= 255 else next((a, n_sym // a) for a in range(2, 256) if n_sym % a == 0 and n_sym // a <= 255)
    streams = [codec.pack_container(h, w, [p]) for p in payloads]
    z = codec.decode_latent(streams, codebook, device=dev)
    return z.cpu().numpy().reshape(len(payloads), n_sym)


@pytest.mark.parametrize('cb', [UNIT, UNEVEN], ids=['unit', 'uneven'])
def test_quantise_equals_scipy_vq(dev, cb):
    rng = np.random.default_rng(1)
    z = (rng.standard_normal((3, 9, 11, 7)) * 6).astype(np.float32)
    mids = ((cb[1:] + cb[:-1]) / 2).astype(np.float32)                       # exact midpoints -> the lower entry
    flat = z.reshape(-1)
    flat[:len(mids)] = mids
    flat[len(mids):len(mids) + len(cb)] = cb
    flat[-6:] = [-1e3, 1e3, cb[0] - 0.75, cb[-1] + 0.75, -40.0, 55.5]       # beyond the codebook
    idx, bad = ops.l3ic_quantise(torch.from_numpy(z).to(dev), torch.from_numpy(cb).to(dev))
    expect = vq(flat, cb)[0].reshape(z.shape).transpose(0, 3, 1, 2).reshape(3, 7, 99)
    assert int(bad.item()) == 0
    assert np.array_equal(idx.cpu().numpy(), expect)


def test_quantise_flags_non_finite(dev):
    z = np.zeros((1, 4, 4, 2), np.float32)
    z[0, 1, 2, 1] = np.nan
    _, bad = ops.l3ic_quantise(torch.from_numpy(z).to(dev), torch.from_numpy(UNIT).to(dev))
    assert int(bad.item()) != 0
    with pytest.raises(codec.L3ICError, match='non-finite'):
        codec.encode_latent(torch.from_numpy(z).to(dev), UNIT)


def test_histogram_and_frequencies_equal_host(dev):
    rng = np.random.default_rng(2)
    n = 32768
    adversarial = np.repeat(np.arange(256), [1] * 200 + [584] * 39 + [576] * 17).astype(np.uint8)
    layers = [rng.permutation(adversarial), _laplace(rng, n, 32), _laplace(rng, n, 256, 40.0),
              np.where(rng.random(n) < 1e-4, 0, 255).astype(np.uint8), rng.integers(0, 256, n).astype(np.uint8),
              np.full(n, 3, np.uint8)]
    payloads, hist, freq = _encode_layers(layers, dev)
    for i, sym in enumerate(layers):
        counts = np.bincount(sym, minlength=256)
        assert np.array_equal(hist[i], counts), i
        assert freq[i].tolist() == ref.normalise(counts), i
        assert payloads[i] == ref.encode_layer(sym), i


@pytest.mark.parametrize('n', [4, 5, 63, 65, 300, 4096, 8192, 16384, 32768, 65025])
def test_payload_bytes_equal_reference(dev, n):
    rng = np.random.default_rng(n)
    layers = [_laplace(rng, n, 32, 1.5), _laplace(rng, n, 2, 0.5), _laplace(rng, n, 256, 30.0),
              np.full(n, 17, np.uint8), rng.integers(0, 256, n).astype(np.uint8)]
    payloads, _, _ = _encode_layers(layers, dev)
    for i, sym in enumerate(layers):
        assert payloads[i] == ref.encode_layer(sym), (n, i)
    alone, _, _ = _encode_layers([layers[0]], dev)                          # a stream coded alone = inside a batch
    assert alone[0] == payloads[0]


def test_gpu_decodes_reference_and_golden_streams(dev):
    rng = np.random.default_rng(3)
    cb = np.linspace(-3, 3, 256).astype(np.float32)
    for n in (4, 65, 4096, 65025):
        layers = [_laplace(rng, n, 32, 1.5), _laplace(rng, n, 256, 20.0), np.full(n, 200, np.uint8)]
        payloads = [ref.encode_layer(s) for s in layers]
        for lanes in (3, 64):                                                # lane counts the encoder never picks
            extra = ref.rans_encode(layers[0], 32, lanes=lanes)
            if len(extra) < n:                                               # (a longer payload is refused)
                payloads.append(extra)
                layers.append(layers[0])
        got = _decode_layers(payloads, n, cb, dev)
        for i, sym in enumerate(layers):
            assert np.array_equal(got[i], cb[sym]), (n, i)                  # exactly codebook[index]
    with np.load(GOLDEN) as g:
        for i in range(len([k for k in g.files if k.startswith('sym')])):
            sym, payload = g['sym{}'.format(i)], g['payload{}'.format(i)].tobytes()
            got = _decode_layers([payload], sym.size, cb, dev)
            assert np.array_equal(got[0], cb[sym]), i


def test_host_decodes_gpu_streams(dev):
    rng = np.random.default_rng(4)
    z = np.clip(np.round(rng.laplace(0, 1.2, (2, 40, 50, 6))), -15, 16).astype(np.float32)
    streams = codec.encode_latent(torch.from_numpy(z).to(dev), UNIT)
    for b, s in enumerate(streams):
        h, w, n, payloads = ref.parse_container(s)
        assert (h, w, n) == (40, 50, 6)
        for layer, p in enumerate(payloads):
            idx = ref.decode_layer(p, h * w, len(UNIT))
            assert np.array_equal(UNIT[idx].reshape(h, w), z[b, :, :, layer])
    back = codec.decode_latent(streams, UNIT, device=dev)
    assert back.dtype == torch.float32 and np.array_equal(back.cpu().numpy(), z)


def test_large_latent_round_trip_and_limit(dev):
    rng = np.random.default_rng(5)
    cb = np.arange(-127, 129, dtype=np.float32)
    z = np.clip(np.round(rng.laplace(0, 3.0, (1, 255, 255, 32))), -127, 128).astype(np.float32)
    z[0, :, :, 5] = 7.0                                                      # an RLE layer
    z[0, :, :, 6] = rng.integers(-127, 129, (255, 255))                      # a RAW layer
    streams = codec.encode_latent(torch.from_numpy(z).to(dev), cb)
    _, _, _, payloads = codec.parse_container(streams[0])
    assert len(payloads[5]) == 3 and len(payloads[6]) == 255 * 255 and payloads[0][0] == 16
    assert np.array_equal(codec.decode_latent(streams, cb, device=dev).cpu().numpy(), z)
    with pytest.raises(codec.L3ICError):
        codec.encode_latent(torch.zeros((1, 256, 4, 2), device=dev), cb)


def test_corrupted_payload_raises(dev):
    rng = np.random.default_rng(6)
    z = np.clip(np.round(rng.laplace(0, 1.0, (2, 64, 64, 3))), -15, 16).astype(np.float32)
    streams = codec.encode_latent(torch.from_numpy(z).to(dev), UNIT)
    h, w, n, payloads = codec.parse_container(streams[1])
    p = bytearray(payloads[2])
    p[len(p) // 2] ^= 0x21                                                   # inside the words
    bad = codec.pack_container(h, w, payloads[:2] + [bytes(p)])
    with pytest.raises(codec.L3ICError, match='Image 1 layer 2'):
        codec.decode_latent([streams[0], bad], UNIT, device=dev)
    trunc = codec.pack_container(h, w, payloads[:2] + [payloads[2][:-2]])
    with pytest.raises(codec.L3ICError, match='Image 0 layer 2'):
        codec.decode_latent([trunc], UNIT, device=dev)


@pytest.mark.parametrize('mode', ['f32', 'bf16'])
@pytest.mark.parametrize('size,bpf', [(128, 5), (256, 8)])
def test_dcn_end_to_end(dev, mode, size, bpf):
    from neural_imaging_amd.models import compression
    from util import natural_images
    ops.set_compute(mode)
    dcn = compression.TwitterDCN(patch_size=size, latent_bpf=bpf, device=dev)
    x = natural_images(1, size, size, seed=size + bpf)
    stream = codec.compress(x, dcn)
    y = codec.decompress(stream, dcn)
    cb = dcn.get_codebook().astype(np.float32)
    z = dcn.compress(x).numpy()
    zq = cb[vq(z.reshape(-1), cb)[0]].reshape(z.shape)
    expect = dcn.decompress(zq).numpy()
    assert y.shape == (1, size, size, 3) and np.array_equal(y, expect)
    h, w, n, _ = codec.parse_container(stream)
    assert (h, w, n) == (size // 8, size // 8, 32)
    y2, stats = codec.compress_n_stats(x, dcn)
    assert np.array_equal(y2, y)
    assert stats['bytes'] == len(stream) and stats['bpp'] == 8 * len(stream) / size / size
    assert np.isfinite(stats['ssim']) and np.isfinite(stats['psnr']) and 0 <= stats['entropy'] <= bpf
    # a batch of two: one stream per image, each the bytes its own latent codes to alone
    xb = np.concatenate([x, natural_images(1, size, size, seed=1)])
    streams = codec.compress_batch(xb, dcn)
    zb = dcn.compress(xb)
    assert len(streams) == 2 and streams == codec.encode_latent(zb, cb)
    assert streams[1] == codec.encode_latent(zb.numpy()[1:], cb)[0]
    assert codec.decompress_batch(streams, dcn).shape == (2, size, size, 3)
    _, bstats = codec.compress_n_stats(xb, dcn)
    assert bstats['bytes'].shape == (2,) and np.array_equal(bstats['bpp'], 8 * bstats['bytes'] / size / size)


def test_coded_laplace_latent_beats_nominal_rate(dev):
    from neural_imaging_amd.models import compression
    dcn = compression.TwitterDCN(patch_size=128, latent_bpf=5, device=dev)
    rng = np.random.default_rng(7)
    z = np.clip(np.round(rng.laplace(0, 1.0, (1, 64, 64, 32))), -15, 16).astype(np.float32)
    p = np.unique(z, return_counts=True)[1] / z.size
    assert 2.2 < -(p * np.log2(p)).sum() < 2.8
    coded = len(codec.encode_latent(torch.from_numpy(z).to(dev), dcn.get_codebook())[0])
    nominal = dcn.compression_stats(patch_size=512)['bytes']
    assert nominal == 64 * 64 * 32 * 5 / 8
    assert coded <= 0.6 * nominal, (coded, nominal)
