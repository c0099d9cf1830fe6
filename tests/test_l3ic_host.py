"""The l3ic bitstream on the host (no GPU): the plain-Python restatement of the payload format (tests/l3ic_ref.py), the pinned
golden streams, and the container / limit logic of neural_imaging_amd.compression.codec."""
import math
import os
import struct

import numpy as np
import pytest

import l3ic_ref as ref
from neural_imaging_amd.compression import codec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'l3ic_streams.npz')


def _laplace(rng, n, k, scale=2.0):
    p = np.exp(-np.abs(np.arange(k) - (k - 1) / 2) / scale)
    return rng.choice(k, n, p=p / p.sum()).astype(np.uint8)


def adversarial_counts():
    """n = 32768: 200 symbols of count 1 and 56 sharing the rest in multiples of 8 -> f sums to 4271, a surplus of 175
    against a largest f of 73 (a rule that took the whole surplus from the maximum would go negative)."""
    c = [1] * 200 + [584] * 39 + [576] * 17
    assert sum(c) == 32768 and len(c) == 256
    return c


# ---- normalisation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('counts,expected', [
    ([3, 1], [3072, 1024]),                                 # exact
    ([1, 2], [1365, 2731]),                                 # deficit 1 -> the largest count
    ([1, 1, 1], [1366, 1365, 1365]),                        # deficit 1, tie -> the lowest index
    ([0, 1, 1, 1, 1, 1, 9995], [0, 1, 1, 1, 1, 1, 4091]),   # surplus 2 from the largest f
    ([1, 1, 1, 1, 5000, 5000], [1, 1, 1, 1, 2046, 2046]),   # surplus 2, ties -> lowest index first, then the next
    ([1, 0, 3], [1024, 0, 3072]),                           # n = 4
])
def test_normalise_pinned(counts, expected):
    assert ref.normalise(counts) == expected


def test_normalise_adversarial_surplus():
    c = adversarial_counts()
    raw = [max(1, v * 4096 // 32768) for v in c]
    assert sum(raw) - 4096 == 175 and max(raw) == 73
    f = ref.normalise(c)
    assert sum(f) == 4096 and min(f) >= 1
    assert f[:200] == [1] * 200 and max(f) - min(f[200:]) <= 1


@pytest.mark.parametrize('counts', [
    adversarial_counts(),
    [1, 65024],                                             # two symbols at 1 : n - 1
    [255] * 256,                                            # all 256 uniform
    [1, 1, 1, 1],                                           # n = 4
    [0] * 100 + [7] + [0] * 50 + [1] * 105,
])
def test_normalise_sums_to_scale(counts):
    f = ref.normalise(counts)
    assert sum(f) == 4096
    assert all((a > 0) == (b > 0) for a, b in zip(f, counts))


def test_normalise_random():
    rng = np.random.default_rng(5)
    for _ in range(200):
        k = int(rng.integers(2, 257))
        c = rng.multinomial(int(rng.integers(4, 65026)), rng.dirichlet(np.full(k, rng.choice([0.05, 0.5, 5.0]))))
        f = ref.normalise(c)
        assert sum(f) == 4096 and all((a > 0) == (b > 0) for a, b in zip(f, c))


# ---- rANS round trip and size bound -----------------------------------------------------------------------------------
def test_lane_rule():
    assert [ref.lanes_for(n) for n in (4, 4095, 4096, 8191, 8192, 16384, 32768, 65025)] == [1, 1, 2, 2, 4, 8, 16, 16]


@pytest.mark.parametrize('k', [2, 32, 256])
@pytest.mark.parametrize('n', [4, 5, 63, 65, 4096, 8192, 16384, 32768, 65025])
def test_reference_round_trip(k, n):
    rng = np.random.default_rng(k * 100003 + n)
    sym = _laplace(rng, n, k, scale=max(0.5, k / 16))
    sym[0], sym[-1] = 0, k - 1                              # at least two distinct symbols, both ends of the range
    payload = ref.rans_encode(sym, k)
    assert payload[0] == ref.lanes_for(n)
    assert np.array_equal(ref.rans_decode(payload, n, k), sym)
    assert np.array_equal(ref.decode_layer(ref.encode_layer(sym, k), n, k), sym)
    # size bound: header + table + states + 2 ceil(ideal_bits / 16) + one partial word per lane
    counts = np.bincount(sym, minlength=k)
    f = ref.normalise(counts)
    lanes = ref.lanes_for(n)
    bound = 3 + ref.table_bytes(f) + 4 * lanes + 2 * math.ceil(ref.ideal_bits(sym, f) / 16) + 2 * lanes
    assert len(payload) <= bound, (len(payload), bound)


@pytest.mark.parametrize('lanes', [1, 3, 7, 64])
def test_decoder_takes_any_lane_count(lanes):
    rng = np.random.default_rng(lanes)
    sym = _laplace(rng, 1000, 32)
    assert np.array_equal(ref.rans_decode(ref.rans_encode(sym, 32, lanes=lanes), 1000, 32), sym)


def test_laplace_rate_close_to_entropy():
    rng = np.random.default_rng(11)
    sym = _laplace(rng, 4096, 32, scale=1.5)
    p = np.bincount(sym, minlength=32) / 4096.0
    h = -(p[p > 0] * np.log2(p[p > 0])).sum()
    assert len(ref.rans_encode(sym, 32)) <= 1.05 * 4096 * h / 8 + 64


# ---- golden streams ---------------------------------------------------------------------------------------------------
def test_golden_streams_decode_and_reencode():
    with np.load(GOLDEN) as g:
        count = len([key for key in g.files if key.startswith('sym')])
        kinds = set()
        for i in range(count):
            sym, k, payload = g['sym{}'.format(i)], int(g['k{}'.format(i)]), g['payload{}'.format(i)].tobytes()
            assert np.array_equal(ref.decode_layer(payload, sym.size, k), sym)
            assert ref.encode_layer(sym, k) == payload
            kinds.add('raw' if len(payload) == sym.size else 'rle' if len(payload) == 3 else 'rans{}'.format(payload[0]))
    assert {'raw', 'rle', 'rans1', 'rans2', 'rans16'} <= kinds


# ---- dispatch, container, limits, corruption --------------------------------------------------------------------------
def test_layer_dispatch():
    assert ref.encode_layer(np.full(100, 7, np.uint8)) == struct.pack('<HB', 100, 7)
    rng = np.random.default_rng(2)
    uniform = rng.integers(0, 256, 500).astype(np.uint8)
    assert ref.encode_layer(uniform) == uniform.tobytes()                     # rANS would not be shorter -> RAW
    skewed = _laplace(rng, 500, 32, scale=1.0)
    p = ref.encode_layer(skewed, 32)
    assert 3 < len(p) < 500 and p[0] == 1
    for payload, n in ((ref.encode_layer(np.full(100, 7, np.uint8)), 100), (uniform.tobytes(), 500), (p, 500)):
        assert ref.decode_layer(payload, n).size == n
    with pytest.raises(ref.FormatError):                                     # a rANS payload is shorter than the layer
        ref.decode_layer(ref.rans_encode(skewed[:20], 32), 20)


def test_container_pack_parse():
    payloads = [b'\x64\x00\x07', bytes(range(16)), b'\x01\x02\x05' + bytes(7)]
    stream = codec.pack_container(4, 4, payloads)
    assert stream[:3] == bytes([4, 4, 3]) and struct.unpack_from('<H', stream, 3)[0] == 6
    assert struct.unpack_from('<3H', stream, 5) == (3, 16, 10)
    assert stream == ref.pack_container(4, 4, payloads)
    h, w, n, got = codec.parse_container(stream)
    assert (h, w, n) == (4, 4, 3) and [bytes(p) for p in got] == payloads
    assert ref.parse_container(stream)[3] == payloads


def test_container_truncated_or_corrupt():
    stream = codec.pack_container(4, 4, [bytes(16), b'\x10\x00\x03'])
    for cut in (0, 2, 4, 6, len(stream) - 1):
        with pytest.raises(codec.L3ICError):
            codec.parse_container(stream[:cut])
    bad = bytearray(stream)
    bad[5] ^= 1                                                               # a layer length
    with pytest.raises(codec.L3ICError):
        codec.parse_container(bytes(bad))
    bad = bytearray(stream)
    bad[3] = 5                                                                # coded (not raw) layer lengths
    with pytest.raises(codec.L3ICError):
        codec.parse_container(bytes(bad))


def test_limits_raise_before_any_device_work():
    with pytest.raises(codec.L3ICError, match='255'):
        codec.encode_latent(np.zeros((1, 256, 4, 2), np.float32), np.arange(4, dtype=np.float32))
    with pytest.raises(codec.L3ICError, match='255'):
        codec.encode_latent(np.zeros((1, 4, 4, 256), np.float32), np.arange(4, dtype=np.float32))
    with pytest.raises(codec.L3ICError, match='at least 4'):
        codec.encode_latent(np.zeros((1, 1, 3, 2), np.float32), np.arange(4, dtype=np.float32))
    with pytest.raises(codec.L3ICError, match='more than 256 centers'):
        codec.encode_latent(np.zeros((1, 4, 4, 2), np.float32), np.arange(257, dtype=np.float32))


def test_truncated_and_bit_flipped_payloads_rejected():
    rng = np.random.default_rng(9)
    sym = _laplace(rng, 4096, 32)
    payload = ref.rans_encode(sym, 32)
    for cut in (1, 2, 5, len(payload) // 2, len(payload) - 2, len(payload) - 1):
        with pytest.raises(ref.FormatError):
            ref.rans_decode(payload[:cut], 4096, 32)
    words_at = 3 + ref.table_bytes(ref.normalise(np.bincount(sym, minlength=32))) + 4 * payload[0]
    for pos in list(range(words_at, len(payload), 97)) + [words_at - 1, 3]:
        bad = bytearray(payload)
        bad[pos] ^= 0x10
        with pytest.raises(ref.FormatError):
            ref.rans_decode(bytes(bad), 4096, 32)
    for head in (bytes([0]), bytes([65])):                                    # lane counts outside 1..64
        with pytest.raises(ref.FormatError):
            ref.rans_decode(head + payload[1:], 4096, 32)
