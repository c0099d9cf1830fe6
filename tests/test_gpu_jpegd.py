"""The JPEG decoder on the GPU (csrc/jpegd.hip through ops.jpeg_decode / ops.jpeg_reconstruct_tables and
compression.jpeg_helpers.decode_batch / decode_coefficients): Pillow's golden files, foreign tables included, byte for byte; round
trips of the encoder here; every route of the synchronisation held to the host program built from the same core (csrc/jpegd.h);
unequal images in one call; damaged streams; the reconstruction with given tables.  Everything exact."""
import numpy as np
import pytest
import torch

import jpeg_cases
import jpeg_ref as ref
import jpegd_cases as cases
import jpegd_ref as dref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

GUARD = 64
DEFAULT_BITS = 2048                 # what subseq_bits = 0 stands for (csrc/jpegd.hip SUBSEQ_DEFAULT)
WORKGROUP = 256                     # threads of the workgroup that synchronises one image (csrc/jpegd.hip SYNC_THREADS)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from neural_imaging_amd import _lib
    _lib.load()
    return torch.device('cuda', 0)


def _decode(streams, subseq_bits, dev):
    """Streams of one geometry through ops.jpeg_decode, guard bytes behind the workspace: (coef (n, -1), status, rounds) numpy."""
    from neural_imaging_amd import _lib
    s0 = streams[0]
    assert all((s.h, s.w, s.hs, s.vs) == (s0.h, s0.w, s0.hs, s0.vs) for s in streams)
    blob = b''.join(s.ecd for s in streams)
    ecd = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s.ecd) for s in streams])]).astype(np.int64)).to(dev)
    huff = torch.from_numpy(np.stack([s.huffman for s in streams])).to(dev)
    size = int(_lib.load().nimg_jpeg_decode_workspace_bytes(len(streams), s0.h, s0.w, s0.hs, s0.vs, len(blob), subseq_bits))
    assert size > 0
    ws = torch.full((size + GUARD,), 0xa5, dtype=torch.uint8, device=dev)
    coef, status, rounds = ops.jpeg_decode(ecd, off, huff, s0.h, s0.w, s0.hs, s0.vs, subseq_bits=subseq_bits, workspace=ws[:size])
    assert (ws[size:] == 0xa5).all(), 'a write behind the workspace'
    return coef.cpu().numpy().reshape(len(streams), -1), status.cpu().numpy(), rounds.cpu().numpy()


def _flat(data):
    return ref.flat_coefficients(dref.real_coefficients(ref.parse(data)))


# ---- 4. golden files ----------------------------------------------------------------------------------------------------------
def test_golden_files_decode_to_pillows_bytes(dev):
    files = cases.files()
    images = jh.decode_batch([f.data for f in files])
    assert isinstance(images, list) and len(images) == len(files)
    for f, y in zip(files, images):
        assert y.dtype == np.uint8 and np.array_equal(y, f.rgb), f.name
    for f in files[::7]:                                  # one file alone: an array with a batch axis; the float form
        assert np.array_equal(jh.decode_batch(f.data)[0], f.rgb), f.name
        y = jh.decode_batch([f.data], as_float=True)
        assert y.dtype == np.float32 and np.array_equal(y[0].view(np.uint32), ref.to_float(f.rgb).view(np.uint32)), f.name


def test_golden_files_give_the_coefficients_of_the_file(dev):
    for f in cases.files():
        coef, tables = jh.decode_coefficients([f.data])
        assert np.array_equal(coef.reshape(-1), _flat(f.data)), f.name
        info, head = ref.parse(f.data), dref.header(f.data)
        assert tables.shape == (1, 3, 64) and all(np.array_equal(tables[0, c], info['qtables'][head['q'][c]]) for c in range(3)), f.name
    f = cases.by_name('smooth_13x21_q75_420/0')
    _, tables = jh.decode_coefficients(f.data)
    assert [jh.jpeg_qf_estimation(jh.libjpeg_qtable(75, c), c) for c in (0, 1)] == \
           [jh.jpeg_qf_estimation(tables[0, c].reshape(8, 8), c) for c in (0, 1)]


# ---- 5. round trip beyond the golden files -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in jpeg_cases.CASES if not c.golden], ids=[c.name for c in jpeg_cases.CASES if not c.golden])
def test_round_trip_of_the_encoder(dev, case):
    x, r = jpeg_cases.build(case), jpeg_cases.reference(case)
    files = jh.encode_batch(x, case.quality, case.subsampling)
    assert files == r.files
    y = jh.decode_batch(files)
    assert y.dtype == np.uint8 and np.array_equal(y, r.decoded)
    image, _ = jh.compress_batch(x, case.quality, subsampling=case.subsampling)
    assert np.array_equal(ref.to_float(y), image) and np.array_equal(y, np.rint(image * np.float32(255)))
    coef, _ = jh.decode_coefficients(files)
    assert np.array_equal(coef.reshape(len(files), -1), r.flat)


# ---- 6. every route of the synchronisation -----------------------------------------------------------------------------------------
ROUTES = ['mixed_64x72_q1_444', 'noise_64x72_q75_422', 'noise_16x24_q100_444', 'checker_16x16_q100_444']


@pytest.fixture(scope='module')
def route_streams():
    out = {}
    for name in ROUTES:
        case = jpeg_cases.by_name(name)
        data = jpeg_cases.reference(case).files[0]
        out[name] = (cases.stream_of(cases.File(name, data, None)), _flat(data))
    return out


@pytest.fixture(scope='module')
def route_host(route_streams):
    results, done = cases.host_results([route_streams[name][0] for name in ROUTES], settings=cases.SETTINGS + (DEFAULT_BITS,))
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    return results


@pytest.mark.parametrize('name', ROUTES)
def test_every_subsequence_length_gives_the_same_coefficients(dev, route_streams, route_host, name):
    stream, want = route_streams[name]
    k = ROUTES.index(name)
    bits = 8 * len(stream.ecd.replace(b'\xff\x00', b'\xff'))
    if name == 'noise_64x72_q75_422':                     # more subsequences than one workgroup has threads: rounds cross its chunks
        assert -(-bits // 32) > WORKGROUP
    if name == 'mixed_64x72_q1_444':
        assert stream.h // 8 * (-(-stream.w // 8)) * 3 / (bits / 1024) > 10        # tens of blocks per 1024-bit subsequence
    for setting in (32, 64, 128, 1024, 0, cases.whole_stream_bits(stream)):            # 0 = the default
        coef, status, rounds = _decode([stream], setting, dev)
        assert status[0] == 0, (setting, status)
        assert np.array_equal(coef[0], want), setting
        if setting == 0:                                  # the default
            subsequences = max(1, -(-bits // DEFAULT_BITS))
            assert rounds[0] == route_host[(k, DEFAULT_BITS)].rounds
        elif setting == cases.whole_stream_bits(stream):
            subsequences = 1
            assert rounds[0] in (0, 1) and rounds[0] == route_host[(k, 0)].rounds
        else:
            subsequences = route_host[(k, setting)].subsequences
            assert subsequences == max(1, -(-bits // setting))
            assert rounds[0] == route_host[(k, setting)].rounds, setting
        assert rounds[0] <= subsequences, setting


# ---- 7. one call, unequal images -----------------------------------------------------------------------------------------------
def test_unequal_images_in_one_call(dev):
    files = [cases.by_name(name) for name in cases.UNEQUAL]
    lengths = [len(cases.stream_of(f).ecd) for f in files]
    assert max(lengths) > 10 * min(lengths)
    assert len({dref.header(f.data)['tables'][1] for f in files}) == 4          # each its own tables
    together = jh.decode_batch([f.data for f in files])
    assert together.shape == (4, 24, 32, 3)
    for i, f in enumerate(files):
        assert np.array_equal(together[i], jh.decode_batch([f.data])[0]), f.name
        assert np.array_equal(together[i], f.rgb), f.name
    coef, _ = jh.decode_coefficients([f.data for f in files])
    for i, f in enumerate(files):
        assert np.array_equal(coef[i].reshape(-1), _flat(f.data)), f.name


def test_mixed_geometries_come_back_in_input_order(dev):
    names = ['mixed_40x56_420_q75_opt', cases.UNEQUAL[2], 'noise_1x1_444_q75_opt', cases.UNEQUAL[0], 'mixed_40x56_420_qt-high',
             'noise_17x33_422_q75_opt']
    files = [cases.by_name(n) for n in names]
    out = jh.decode_batch([f.data for f in files])
    assert isinstance(out, list) and len(out) == len(files)
    for f, y in zip(files, out):
        assert y.shape == f.rgb.shape and np.array_equal(y, f.rgb), f.name
    dev_out = jh.decode_batch([f.data for f in files], device_output=True)
    assert all(t.is_cuda and np.array_equal(t.cpu().numpy(), f.rgb) for f, t in zip(files, dev_out))


# ---- 8. damaged streams ------------------------------------------------------------------------------------------------------------
def test_damaged_streams_report_the_host_programs_status(dev):
    """The damaged streams of test_jpegd_host.py (same seeds), grouped by geometry with one valid stream in front: status and, where
    the damage leaves a decodable stream, coefficients are the host program's; nothing is written outside the workspace."""
    damaged, valid = cases.damaged_streams(), cases.valid_streams()
    host, done = cases.host_results(damaged, settings=(0,))
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    groups = {}
    for k, s in enumerate(damaged):
        groups.setdefault((s.h, s.w, s.hs, s.vs), []).append(k)
    seen = 0
    for key, members in groups.items():
        good = next(j for j, s in enumerate(valid) if (s.h, s.w, s.hs, s.vs) == key)
        coef, status, rounds = _decode([valid[good]] + [damaged[k] for k in members], 0, dev)
        assert status[0] == 0 and np.array_equal(coef[0], _flat(cases.files()[good].data)), key
        for row, k in enumerate(members, 1):
            assert status[row] == host[(k, 0)].status, damaged[k].name
            if status[row] == 0:
                assert np.array_equal(coef[row], host[(k, 0)].coef), damaged[k].name
            seen += 1
    assert seen == len(damaged)


def test_decode_batch_names_the_damaged_files(dev):
    damaged, valid = cases.damaged_streams(), cases.valid_streams()
    host, done = cases.host_results(damaged, settings=(0,))
    assert done.returncode == 0
    name = 'mixed_40x56_420_q75_opt'
    original = cases.by_name(name)
    picks = []
    for k, s in enumerate(damaged):
        if s.name.startswith(name + '|') and host[(k, 0)].status:
            try:
                jh.parse_header(cases.file_of(s, original.data))
            except ValueError:
                continue                                  # damage that made a marker: refused on the host already
            picks.append(k)
    assert len(picks) >= 3
    picks = picks[:5]
    batch = [cases.file_of(damaged[picks[0]], original.data), original.data] + [cases.file_of(damaged[k], original.data) for k in picks[1:]]
    bad = [0] + list(range(2, len(batch)))
    with pytest.raises(ValueError) as e:
        jh.decode_batch(batch)
    assert 'file(s) {}:'.format(bad) in str(e.value)
    for i, k in zip(bad, picks):
        assert '{}: status {} '.format(i, host[(k, 0)].status) in str(e.value)
    files = cases.files()                                 # and the decoder is as exact as before
    for f, y in zip(files, jh.decode_batch([f.data for f in files])):
        assert np.array_equal(y, f.rgb), f.name


# ---- 9. reconstruction with given tables -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['smooth_17x33_q95_444', 'noise+smooth+constant+checker_16x24_q75_422', 'mixed_40x56_q1_420'])
def test_reconstruct_tables_equals_reconstruct(dev, name):
    case = jpeg_cases.by_name(name)
    assert case.golden
    hs, vs = ops.jpeg_subsampling(case.subsampling)
    x = torch.from_numpy(np.array(jpeg_cases.build(case))).to(dev)
    coef = ops.jpeg_transform(x, case.quality, hs, vs)
    want = ops.jpeg_reconstruct(coef, case.h, case.w, case.quality, hs, vs)
    tables = np.stack([jh.libjpeg_qtable(case.quality, c).reshape(64) for c in (0, 1, 1)]).astype(np.uint16)
    qt = torch.from_numpy(np.repeat(tables[None], len(x), 0).view(np.int16)).to(dev)
    as_float = ops.jpeg_reconstruct_tables(coef, case.h, case.w, qt, hs, vs)
    as_bytes = ops.jpeg_reconstruct_tables(coef, case.h, case.w, qt, hs, vs, out_u8=True)
    assert as_float.dtype == torch.float32 and torch.equal(as_float.view(torch.int32), want.view(torch.int32))
    assert as_bytes.dtype == torch.uint8 and np.array_equal(as_bytes.cpu().numpy(), jpeg_cases.golden()[name][2])
    assert np.array_equal(ref.to_float(as_bytes.cpu().numpy()), want.cpu().numpy())       # numpy's float32 division is the kernel's
