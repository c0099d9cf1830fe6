"""Every route of the l3ic codec (csrc/l3ic.hip) on the GPU, byte for byte against tests/l3ic_ref.py.  Cases, their ids and the
reference halves: tests/l3ic_cases.py; its self-test, which also counts the routes: tests/test_l3ic_cases.py.  Everything is
np.array_equal or bytes equality - there is no tolerance in this module.  The entry points are called through _lib with 0xa5 guard
bytes behind every buffer the wrappers of ops.py would allocate (out, lengths, hist, freq, workspace; z and err; idx and the flag);
the guards, and the part of `out` behind the last payload, must come back untouched.

  test id                                   kernel                 branch reached
  ----------------------------------------  ---------------------  -----------------------------------------------------------------
  encode_routes[n4 .. n17, n103]            l3ic_encode_kernel     deficit with the maximum count tied in two lanes (symbols 5 | 200,
                                                                   200 | 201 | 250), deficit of 1, exact sum; RAW before the loop
                                                                   (max_words < 0) at n = 4, 7, 11, 17, 103; max_words = 0 at n = 12;
                                                                   payload of n - 1 (rANS), n and n + 1 bytes (RAW inside the loop);
                                                                   RLE at n = 4
  encode_routes[n300]                       l3ic_encode_kernel     256 symbols: RAW inside the loop, deficit of 152
  encode_routes[n4096]                      l3ic_encode_kernel     table bytes: 127 | 128 (the varint switch), zero frequencies inside
                                                                   a..b, a = 0 with b = 255, b = a + 1, f = {1, 4095} and {4095, 1},
                                                                   symbols starting on slots 64 and 2048; L = 2; nine streams
  encode_routes[n4113, n4115, n4129,        l3ic_encode_kernel     the surplus bisection at the smallest n of the searched family:
                n4147]                                             surplus of 1, left > 0 with the cut level in three lanes, left == 0,
                                                                   two levels coming down
  encode_routes[n4095 .. n65535]            l3ic_encode_kernel     both sides of every switch of the lane rule (L = 1, 2, 4, 8, 16), a
                                                                   ragged last step at the odd sizes; the 8-fold unrolled staging loop
                                                                   and its tail; at 32768 the adversarial histogram (surplus 175, left
                                                                   24, three levels), at 65535 255 singletons (surplus 239), RLE and RAW
  (each of the above)                       l3ic_scan_kernel,      per = 1; streams of unequal length packed back to back
                                            l3ic_gather_kernel
  (each of the above)                       l3ic_decode_kernel     RAW, RLE and rANS with the encoder's lane counts; the decode table
                                                                   of each table-byte case
  many_streams[1024 | 1025 | 2500]          l3ic_scan_kernel       per = 1, 2, 3: several streams per thread, threads with j0 >= streams
                                                                   (511 and 190 of them), hist / freq null; consecutive lengths differ
                                            l3ic_decode_kernel     n * c = 1024, 1025 and 2500 streams in one launch, c = 256, 25, 250
  foreign_streams[...]                      l3ic_decode_kernel     L = 1, 3, 5, 63, 64 at n = 600 (T = 10 with ragged steps of 33 and
                                                                   24); the shortest layer of each lane count, n = 4 L + 6 (T = 5); a
                                                                   forged single-symbol table with f = 4096; first-slot marks on row
                                                                   boundaries (every row at once), {1, 4095}, {4095, 1} at L = 2, 3, 64
  damaged_built                             l3ic_decode_kernel     each NIMG_L3IC_E_* bit alone, ten combinations, payloads of 0, 1 and
                                                                   2 bytes, the three exits (header, table, body); a valid stream first
  damaged_below_the_lane_count              l3ic_decode_kernel     n_sym = 40 under L = 64 and 8: lanes that hold a state and no symbol
  damaged_family[base0 | base1 | base2]     l3ic_decode_kernel     70 bit flips and 9 - 10 truncations of each of three payloads
                                                                   (L = 1, 2 and a foreign 64)
  quantise[...]                             l3ic_quantise_kernel   n_sym = 1, 63, 64, 65, 200 with three images (tail workgroups);
                                                                   c = 1, 3, 255, 256; k = 1, 2, 256; sorted, unsorted and repeated
                                                                   code-books; midpoints, both ends, -0.0, +-3e38; a non-finite value
                                                                   in the first pixel, the last pixel and a tail workgroup
  quantise_at_2048_features                 l3ic_quantise_kernel   128 KiB of dynamic LDS through ops.l3ic_quantise; c = 2049 refused

A rANS payload holds 4 L bytes of states and is shorter than n_sym, so n_sym > 4 L + 5: a VALID stream with n_sym < L does not exist
(tests/test_l3ic_cases.py asserts it); the damaged cases reach the decoder's body in that state."""
import time

import numpy as np
import pytest
import torch

import l3ic_cases as cases
import l3ic_ref as ref
from neural_imaging_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 256
CODEBOOK = (np.arange(256, dtype=np.float32) * np.float32(0.25) - np.float32(7)).astype(np.float32)          # all entries differ
_T0 = [0.0]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()           # fail loudly if the HIP library is missing
    _T0[0] = time.monotonic()
    yield torch.device('cuda', 0)
    print('l3ic routes: module wall time {:.1f} s'.format(time.monotonic() - _T0[0]))        # (shown with pytest -s)


def _guarded(nbytes, dev):
    """(the whole buffer, filled with 0xa5; its first nbytes) - the buffer is checked with _intact afterwards."""
    whole = torch.full((nbytes + GUARD,), 0xa5, dtype=torch.uint8, device=dev)
    return whole, whole[:nbytes]


def _intact(whole, nbytes, what):
    assert bool((whole[nbytes:] == 0xa5).all()), 'a write behind ' + what


def _encode(layers, dev, want_stats=True):
    """nimg_l3ic_encode over equally long layers with guards everywhere: ([payload bytes], lengths, hist, freq) as numpy."""
    from neural_imaging_amd import _lib
    idx = torch.from_numpy(np.ascontiguousarray(np.stack(layers))).to(dev)
    streams, n_sym = idx.shape
    size = int(_lib.load().nimg_l3ic_workspace_bytes(streams, n_sym))
    assert size > 0
    ws_all, ws = _guarded(size, dev)
    out_all, out = _guarded(streams * n_sym, dev)
    len_all, lengths = _guarded(4 * streams, dev)
    hist_all, hist = _guarded(1024 * streams, dev) if want_stats else (None, None)
    freq_all, freq = _guarded(1024 * streams, dev) if want_stats else (None, None)
    _lib.call('nimg_l3ic_encode', ops._p(idx), streams, n_sym, ops._p(out), ops._p(lengths), ops._p(hist), ops._p(freq), ops._p(ws),
              size, ops._stream())
    lengths = lengths.cpu().numpy().view(np.uint32).astype(np.int64)
    assert lengths.shape == (streams,) and int(lengths.max()) <= n_sym
    total = int(lengths.sum())
    blob = out.cpu().numpy()
    assert np.all(blob[total:] == 0xa5), 'a write behind the last payload'
    _intact(ws_all, size, 'the workspace')
    _intact(out_all, streams * n_sym, 'out')
    _intact(len_all, 4 * streams, 'lengths')
    if want_stats:
        _intact(hist_all, 1024 * streams, 'hist')
        _intact(freq_all, 1024 * streams, 'freq')
        hist, freq = (t.cpu().numpy().view(np.uint32).reshape(streams, 256) for t in (hist, freq))
    ends = np.concatenate([[0], np.cumsum(lengths)])
    blob = blob.tobytes()
    return [blob[ends[i]:ends[i + 1]] for i in range(streams)], lengths, hist, freq


def _decode(payloads, shape, k, dev):
    """nimg_l3ic_decode of stream s = image s // c, layer s % c with guards behind z and err: (z (n, h * w, c), err (n * c,))."""
    from neural_imaging_amd import _lib
    n, h, w, c = shape
    assert len(payloads) == n * c
    lengths = np.array([len(p) for p in payloads], np.int64)
    offsets = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    data = torch.from_numpy(np.frombuffer(b''.join(payloads) + b'\xa5' * 16, np.uint8).copy()).to(dev)
    meta = torch.from_numpy(np.concatenate([offsets, lengths]).astype(np.int32)).to(dev)
    cb = torch.from_numpy(CODEBOOK[:k].copy()).to(dev)
    z_all, z = _guarded(4 * n * h * w * c, dev)
    err_all, err = _guarded(4 * n * c, dev)
    _lib.call('nimg_l3ic_decode', ops._p(data), ops._p(meta[:n * c]), ops._p(meta[n * c:]), ops._p(cb), k, ops._p(z), ops._p(err), n, h, w,
              c, ops._stream())
    _intact(z_all, 4 * n * h * w * c, 'z')
    _intact(err_all, 4 * n * c, 'err')
    return z.cpu().numpy().view(np.float32).reshape(n, h * w, c), err.cpu().numpy().view(np.uint32).astype(np.int64)


def _check_decoded(decs, z, err, first=0):
    """Streams `first` .. of one image-major call (n = 1): the status is l3ic_ref.decode_status; where it is 0 the latent is
    codebook[ref.decode_layer]."""
    for s, d in enumerate(decs, first):
        want = ref.decode_status(d.payload, d.n, d.k)
        assert err[s] == want, (d.id, int(err[s]), want)
        if want == 0:
            sym = ref.decode_layer(d.payload, d.n, d.k)
            if d.sym is not None:
                assert np.array_equal(sym, d.sym), d.id
            assert np.array_equal(z[0, :, s], CODEBOOK[sym]), d.id


# ---- encoder: every route, then the decoder on what it wrote ---------------------------------------------------------------------
GROUPS = cases.encoder_groups()


@pytest.mark.parametrize('n', sorted(GROUPS), ids=['n{}'.format(n) for n in sorted(GROUPS)])
def test_encode_routes(dev, n):
    group = GROUPS[n]
    payloads, lengths, hist, freq = _encode([c.sym for c in group], dev)
    for i, c in enumerate(group):
        counts = np.bincount(c.sym, minlength=256)
        assert np.array_equal(hist[i], counts), c.id
        assert freq[i].tolist() == ref.normalise(counts), c.id
        want = cases.reference_payload(c.sym.tobytes())
        assert lengths[i] == len(want), (c.id, int(lengths[i]), len(want))
        assert payloads[i] == want, c.id
    z, err = _decode(payloads, (1, 1, n, len(group)), 256, dev)
    assert not err.any(), err
    for i, c in enumerate(group):
        assert np.array_equal(z[0, :, i], CODEBOOK[c.sym]), c.id
    if len(group) > 1:                                        # a stream coded alone = inside the batch, without the statistics
        alone, _, _, _ = _encode([group[-1].sym], dev, want_stats=False)
        assert alone[0] == payloads[-1]


# ---- many streams: the scan with several streams per thread -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def pool_alone(dev):
    """Every layer of the pool coded alone through ops.l3ic_encode: {layer bytes: payload}."""
    out = {}
    for layers in cases.stream_pool().values():
        for sym in layers:
            data, lengths, hist, freq = ops.l3ic_encode(torch.from_numpy(sym[None]).to(dev))
            assert hist is None and freq is None
            out[sym.tobytes()] = data[:int(lengths[0])].cpu().numpy().tobytes()
            assert out[sym.tobytes()] == cases.reference_payload(sym.tobytes())
    return out


@pytest.mark.parametrize('count,c', [(1024, 256), (1025, 25), (2500, 250)])
def test_many_streams(dev, pool_alone, count, c):
    idx, want = cases.many_streams(count)
    payloads, lengths, _, _ = _encode(list(idx), dev, want_stats=False)
    assert lengths.tolist() == [len(p) for p in want]
    assert b''.join(payloads) == b''.join(want)               # the packed blob
    for s in range(count):
        assert payloads[s] == pool_alone[idx[s].tobytes()], s
    z, err = _decode(payloads, (count // c, 4, 4, c), 256, dev)
    assert not err.any()
    assert np.array_equal(z, CODEBOOK[idx].reshape(count // c, c, 16).transpose(0, 2, 1))
    data = torch.from_numpy(np.frombuffer(b''.join(want), np.uint8).copy()).to(dev)          # the same through the wrapper
    meta = torch.from_numpy(np.concatenate([np.concatenate([[0], np.cumsum(lengths)[:-1]]), lengths]).astype(np.int32)).to(dev)
    z2, err2 = ops.l3ic_decode(data, meta[:count], meta[count:], torch.from_numpy(CODEBOOK).to(dev), (count // c, 4, 4, c))
    assert not bool(err2.any()) and np.array_equal(z2.cpu().numpy().reshape(count // c, 16, c), z)


# ---- decoder: valid streams the encoder never writes ------------------------------------------------------------------------------
FOREIGN = {}
for _d in cases.foreign_cases():
    FOREIGN.setdefault((_d.n, _d.k), []).append(_d)


@pytest.mark.parametrize('key', sorted(FOREIGN), ids=['n{}-k{}'.format(*key) for key in sorted(FOREIGN)])
def test_foreign_streams(dev, key):
    n, k = key
    decs = FOREIGN[key]
    assert all(len(d.payload) < n for d in decs)
    z, err = _decode([d.payload for d in decs], (1, 1, n, len(decs)), k, dev)
    assert not err.any(), err
    _check_decoded(decs, z, err)
    for i, d in enumerate(decs):
        assert np.array_equal(z[0, :, i], CODEBOOK[d.sym]), d.id


# ---- decoder: damaged payloads ---------------------------------------------------------------------------------------------------------
def _with_valid_first(decs, good, sym, dev):
    n, k = decs[0].n, decs[0].k
    z, err = _decode([good] + [d.payload for d in decs], (1, 1, n, len(decs) + 1), k, dev)
    assert err[0] == 0 and np.array_equal(z[0, :, 0], CODEBOOK[sym]), 'the valid stream in front'
    _check_decoded(decs, z, err, first=1)
    return err[1:]


def test_damaged_built(dev):
    n, k, good, sym = cases.damaged_bases()[0]
    decs = cases.damaged_built()
    err = _with_valid_first(decs, good, sym, dev)
    alone = set()
    for d, e in zip(decs, err):
        named = d.id.split('/')[0]
        if named == 'valid':
            assert e == 0, d.id
        elif named != 'any':                                  # the bits by name, not only by the restatement
            assert e == sum(bit for bit, name in ref.E_NAMES.items() if name in named.split('+')), (d.id, int(e))
        if bin(int(e)).count('1') == 1:
            alone.add(int(e))
    assert alone == set(ref.E_NAMES)                          # every NIMG_L3IC_E_* bit reported alone at least once
    assert sum(1 for e in err if bin(int(e)).count('1') >= 2) >= 3


def test_damaged_below_the_lane_count(dev):
    decs = cases.damaged_small()
    good = ref.rans_encode(np.array([0] * 35 + [1] * 5, np.uint8), 2, lanes=3)
    assert len(good) < 40
    err = _with_valid_first(decs, good, np.array([0] * 35 + [1] * 5, np.uint8), dev)
    assert np.count_nonzero(err) == 3 and err[-1] == 0


@pytest.mark.parametrize('base', [0, 1, 2], ids=['base0', 'base1', 'base2'])
def test_damaged_family(dev, base):
    n, k, good, sym = cases.damaged_bases()[base]
    decs = [d for b, d in cases.damaged_family() if b == base]
    assert len(decs) >= 75
    err = _with_valid_first(decs, good, sym, dev)
    assert np.count_nonzero(err) >= 70


# ---- quantiser ------------------------------------------------------------------------------------------------------------------------
def _quantise(q, dev):
    from neural_imaging_amd import _lib
    b, h, n_sym, c = q.z.shape
    z = torch.from_numpy(q.z).to(dev)
    cb = torch.from_numpy(q.cb).to(dev)
    idx_all, idx = _guarded(b * c * n_sym, dev)
    flag_all, flag = _guarded(4, dev)
    flag.zero_()
    _lib.call('nimg_l3ic_quantise', ops._p(z), ops._p(cb), q.cb.size, ops._p(idx), ops._p(flag), b, h, n_sym, c, ops._stream())
    _intact(idx_all, b * c * n_sym, 'idx')
    _intact(flag_all, 4, 'the flag')
    return idx.cpu().numpy().reshape(b, c, n_sym), int(flag.cpu().numpy().view(np.int32)[0])


QUANT = [q for q in cases.quantiser_cases() if q.z.shape[3] <= 1008]


@pytest.mark.parametrize('q', QUANT, ids=[q.id for q in QUANT])
def test_quantise(dev, q):
    idx, flag = _quantise(q, dev)
    assert np.array_equal(idx, cases.quantise_reference(q.z, q.cb))
    assert (flag != 0) == q.bad


def test_quantise_at_2048_features(dev):
    """c = 2048, the documented bound: 64 c = 128 KiB of dynamic LDS, which nimg_l3ic_quantise launches without raising the
    kernel's limit (encode and decode do raise theirs).  Measured on gfx950: the launch works as written and equals the reference."""
    q = next(q for q in cases.quantiser_cases() if q.z.shape[3] == 2048)
    idx, bad = ops.l3ic_quantise(torch.from_numpy(q.z).to(dev), torch.from_numpy(q.cb).to(dev))
    assert int(bad.item()) == 0
    assert np.array_equal(idx.cpu().numpy(), cases.quantise_reference(q.z, q.cb))
    with pytest.raises(RuntimeError):                         # one beyond the bound is refused before any launch
        ops.l3ic_quantise(torch.zeros((1, 1, 4, 2049), device=dev), torch.from_numpy(q.cb).to(dev))
