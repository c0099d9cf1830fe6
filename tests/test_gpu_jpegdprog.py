"""Reading progressive JPEG files on the GPU (csrc/jpegd_prog.hip through ops.jpeg_decode_progressive and decode_batch /
decode_coefficients / transcode_batch with allow_progressive): the Pillow files, the files of two further scan scripts and synthetic
tensors held to the host program built from the same core (csrc/jpegdprog.h) - coefficients, status and synchronisation rounds at
every subsequence length; pixels held to Pillow's and to the baseline twin; round trips and transcoding; batching; damaged streams;
refusals.  Everything exact."""
import ctypes
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

import jpeg_ref as ref
import jpegdprog_cases as cases
import jpegdprog_ref as dpref
import jpegprog_cases as pc
from neural_imaging_amd import _lib, ops
from neural_imaging_amd.compression import jpeg_helpers as jh

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xa5
DEFAULT_BITS = 512                  # what subseq_bits = 0 stands for (csrc/jpegd_prog.hip PROG_SUBSEQ_DEFAULT)
ERR_ARG = -1                        # include/nimg.h NIMG_ERR_ARG
WORKGROUP = 256                     # threads of the workgroup that decodes one first scan (csrc/jpegd_prog.hip FIRST_THREADS)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    _lib.load()
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def host():
    """The host program over every valid and every damaged file, once: {file name: Host}."""
    files = cases.valid_files() + cases.damaged_files()
    out, done = cases.host_results(files, settings=cases.SETTINGS + (DEFAULT_BITS,), sanitize=False)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    return {f.name: h for f, h in zip(files, out)}


def _guarded(count, dtype, dev):
    whole = torch.full((count * dtype.itemsize + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
    return whole, whole[GUARD:GUARD + count * dtype.itemsize].view(dtype)


def _intact(whole):
    return bool((whole[:GUARD] == FILL).all()) and bool((whole[-GUARD:] == FILL).all())


def _groups(files):
    """Files of equal geometry, interval and script together: what one library call takes."""
    out = OrderedDict()
    for f in files:
        out.setdefault((f.h, f.w, f.hs, f.vs, f.ri, f.script), []).append(f)
    return list(out.values())


def _decode(group, subseq_bits, dev, script_rows=None, short=0, expect=0):
    """One call of the library on files of one group, every output and the workspace between guard bytes -> (coef (n, -1), status,
    rounds (n, scans)) numpy, or the outputs as they were left when the call is expected to be refused."""
    f0, n, ns = group[0], len(group), len(group[0].script)
    segs = [s for f in group for s in f.segments]
    blob = b''.join(segs)
    ecd = torch.from_numpy(np.frombuffer(blob if blob else b'\0', np.uint8).copy()).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in segs])]).astype(np.int64)).to(dev)
    huff = torch.from_numpy(np.stack([np.stack(f.tables) for f in group])).to(dev)
    rows = np.ascontiguousarray(cases.dpref_rows(f0.script) if script_rows is None else script_rows, np.int32)
    lib = _lib.load()
    size = int(lib.nimg_jpeg_decode_progressive_workspace_bytes(n, f0.h, f0.w, f0.hs, f0.vs, f0.ri, ns, len(blob), subseq_bits))
    assert size > 0
    nb = ops.jpeg_geometry(f0.h, f0.w, f0.hs, f0.vs)[0]
    wc, coef = _guarded(n * nb * 64, torch.int16, dev)
    wst, status = _guarded(n, torch.int32, dev)
    wr, rounds = _guarded(n * ns, torch.int32, dev)
    ww, ws = _guarded(size - short, torch.uint8, dev)
    rc = lib.nimg_jpeg_decode_progressive(ecd.data_ptr(), off.data_ptr(), rows.ctypes.data, ns, huff.data_ptr(), n, f0.h, f0.w, f0.hs, f0.vs, f0.ri,
                                          subseq_bits, coef.data_ptr(), status.data_ptr(), rounds.data_ptr(), ws.data_ptr(), size - short,
                                          ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == expect, rc
    assert all(_intact(w) for w in (wc, wst, wr, ww)), 'a write outside an output or the workspace'
    return coef.cpu().numpy().reshape(n, -1), status.cpu().numpy(), rounds.cpu().numpy().reshape(n, ns)


# ---- coefficients, status and rounds -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', cases.SETTINGS)
def test_every_valid_file_equals_the_host_program(dev, host, setting):
    files = cases.valid_files()
    assert len(files) == 72 + 30 + 5
    seam = False
    for group in _groups(files):
        bits = max(cases.whole_bits(f) for f in group) if setting == 0 else setting
        coef, status, rounds = _decode(group, bits, dev)
        for i, f in enumerate(group):
            h = host[f.name]
            assert status[i] == 0 == h.status[setting], (f.name, status[i])
            assert np.array_equal(coef[i], f.expected) and np.array_equal(coef[i], h.coef[setting]), f.name
            assert rounds[i].tolist() == h.rounds[setting], (f.name, rounds[i].tolist(), h.rounds[setting])
            seam |= max(8 * len(s) for s in f.segments) > WORKGROUP * setting > 0 and max(h.rounds[setting]) > 0
    if setting == 32:
        assert seam                                    # a first scan of more than one chunk of subsequences that took rounds


def test_the_default_subsequence_length(dev, host):
    group = [f for f in cases.valid_files() if f.name == 'smooth_136x200_q95_444|0|std']
    coef, status, rounds = _decode(group, 0, dev)
    assert status[0] == 0 and np.array_equal(coef[0], group[0].expected) and rounds[0].tolist() == host[group[0].name].rounds[DEFAULT_BITS]
    assert max(rounds[0]) >= 1


# ---- pixels ------------------------------------------------------------------------------------------------------------------------------
def _twin(case):
    """encode_batch's optimised baseline files of a case's images."""
    return jh.encode_batch(pc.build(case), case.quality, case.subsampling, optimize=True, qtables=pc.qtables(case), restart_interval=case.ri)


def test_pixels_are_pillows_and_the_baseline_twins(dev):
    crcs = cases.stored()[1]
    files = [f for f in cases.golden_files() + cases.script_files() if not f.slow]
    images = jh.decode_batch([f.data for f in files], allow_restart=True, allow_progressive=True)
    assert len(images) == len(files) == 71 + 30
    for f, y in zip(files, images):
        assert y.dtype == np.uint8 and y.shape == (f.h, f.w, 3) and zlib.crc32(np.ascontiguousarray(y).tobytes()) == crcs[f.name], f.name
    by = {f.name: y for f, y in zip(files, images)}
    for name in ('mixed_37x53_q75_420_ri2', 'mixed_37x53_q75_444_ri0', 'mixed_40x56_three_422', 'mixed_128x192_q75_420_ri5',
                 'g_noise+smooth+constant+checker_16x24_q75_422', 'corr_32x160_q100_420'):
        twins = jh.decode_batch(_twin(pc.by_name(name)), allow_restart=True)
        for i, y in enumerate(twins):
            assert np.array_equal(by['{}|{}|std'.format(name, i)], y), name
        for s in ('A', 'B'):
            if name in cases.SCRIPT_CASES:
                assert np.array_equal(by['{}|0|{}'.format(name, s)], twins[0]), (name, s)
    y = jh.decode_batch(files[3].data, as_float=True, allow_progressive=True)
    assert y.dtype == np.float32 and np.array_equal(y[0].view(np.uint32), ref.to_float(by[files[3].name]).view(np.uint32))


# ---- round trip and transcoding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('subsampling', ('4:4:4', '4:2:2', '4:2:0'))
@pytest.mark.parametrize('ri', (0, 3))
def test_round_trip_of_the_progressive_writer(dev, subsampling, ri):
    case = pc.by_name('mixed_37x53_q75_{}_ri{}'.format(subsampling.replace(':', ''), ri))
    x = pc.build(case)
    files = jh.encode_batch(x, case.quality, subsampling, restart_interval=ri, progressive=True)
    coef, tables = jh.decode_coefficients(files, allow_restart=True, allow_progressive=True)
    hs, vs = ref.SUBSAMPLING[subsampling]
    want = ops.jpeg_transform(torch.from_numpy(x.copy()).to(dev), case.quality, hs, vs)
    assert np.array_equal(coef, want.cpu().numpy()) and np.array_equal(coef.reshape(len(x), -1), pc.reference(case).flat)
    assert all(np.array_equal(tables[0, c].reshape(8, 8), jh.libjpeg_qtable(75, min(c, 1))) for c in range(3))


def test_transcoding(dev):
    for name in ('mixed_37x53_q75_420_ri2', 'mixed_37x53_q75_422_ri0', 'mixed_40x56_three_422', 'g_noise+smooth+constant+checker_16x24_q75_422',
                 'corr_32x160_q100_420', 'mixed_128x192_q75_420_ri5'):
        case = pc.by_name(name)
        P = pc.golden()[name]
        assert jh.transcode_batch(P, allow_restart=True, allow_progressive=True) == _twin(case), name            # jpegtran -optimize
        assert jh.transcode_batch(P, allow_restart=True, allow_progressive=True, progressive=True) == P, name
        if name in cases.SCRIPT_CASES:                     # any script comes back as the simple progression of the same coefficients
            other = [cases.stored()[0]['{}|{}'.format(name, s)] for s in ('A', 'B')]
            assert jh.transcode_batch(other, allow_restart=True, allow_progressive=True, progressive=True) == [P[0], P[0]], name
            assert jh.transcode_batch(other, allow_restart=True, allow_progressive=True) == [_twin(case)[0]] * 2, name


# ---- batching ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def calls(monkeypatch):
    """The entry-point names _lib.call is given, in order; the calls go through."""
    names, call = [], _lib.call

    def recorded(name, *args):
        names.append(name)
        return call(name, *args)
    monkeypatch.setattr(_lib, 'call', recorded)
    return names


def test_unequal_images_in_one_call(dev, host):
    name = 'g_noise+smooth+constant+checker_16x24_q75_422'
    group = [f for f in cases.golden_files() if f.name.startswith(name + '|')]
    assert len(group) == 4 and len({len(b''.join(f.segments)) for f in group}) > 1
    for setting in (32, DEFAULT_BITS):
        coef, status, rounds = _decode(group, setting, dev)
        for i, f in enumerate(group):
            alone = _decode([f], setting, dev)
            assert status[i] == 0 and np.array_equal(coef[i], f.expected) and np.array_equal(coef[i], alone[0][0]), f.name
            assert rounds[i].tolist() == alone[2][0].tolist() == host[f.name].rounds[setting], f.name


def test_mixed_files_come_back_in_input_order_with_one_call_per_group(dev, calls):
    stored = cases.stored()[0]
    a, b = 'mixed_37x53_q75_420_ri0', 'mixed_40x56_three_422'
    base = {n: _twin(pc.by_name(n))[0] for n in (a, b)}
    files = [stored[a + '|A'], base[b], pc.golden()[a][0], stored[b + '|B'], base[a], stored[a + '|B'], pc.golden()[b][0], stored[b + '|A'],
             pc.golden()[a][0]]
    del calls[:]
    images = jh.decode_batch(files, allow_progressive=True)
    # eight groups: (37x53 | 40x56) x (baseline | standard | A | B); the standard 37x53 file is there twice
    assert calls == ['nimg_jpeg_decode_progressive', 'nimg_jpeg_decode_restart', 'nimg_jpeg_decode_progressive',
                     'nimg_jpeg_decode_progressive', 'nimg_jpeg_decode_restart', 'nimg_jpeg_decode_progressive',
                     'nimg_jpeg_decode_progressive', 'nimg_jpeg_decode_progressive'] + ['nimg_jpeg_reconstruct_tables'] * 8
    want = {n: jh.decode_batch(base[n])[0] for n in (a, b)}
    assert [y.shape for y in images] == [(37, 53, 3) if k in (0, 2, 4, 5, 8) else (40, 56, 3) for k in range(9)]
    for k, y in enumerate(images):
        assert np.array_equal(y, want[a if k in (0, 2, 4, 5, 8) else b]), k
    del calls[:]
    coef, _ = jh.decode_coefficients([pc.golden()[a][0]] * 3, allow_progressive=True)
    assert calls == ['nimg_jpeg_decode_progressive'] and coef.shape[0] == 3
    with pytest.raises(ValueError, match='one geometry and scan script'):
        jh.decode_coefficients([stored[a + '|A'], stored[a + '|B']], allow_progressive=True)


# ---- damaged streams -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('setting', (32, DEFAULT_BITS, 0))
def test_damaged_streams_end_with_the_host_programs_status(dev, host, setting):
    files = cases.damaged_files()
    assert len(files) >= 300
    for group in _groups(files):
        for f in group:                                    # every file alone: tables differ, and a status is one image's
            bits = cases.whole_bits(f) if setting == 0 else setting
            coef, status, rounds = _decode([f], bits, dev)
            h = host[f.name]
            assert status[0] == h.status[setting], (f.name, status[0], h.status[setting])
            assert rounds[0].tolist() == h.rounds[setting], f.name
            if status[0] == 0:
                assert np.array_equal(coef[0], h.coef[setting]), f.name


def test_decode_batch_names_the_damaged_files_and_the_bits(dev, host):
    good = pc.golden()['mixed_37x53_q75_420_ri2'][0]
    hd = jh.parse_header(good, True, True)
    cut = hd.scans[2].ecd_offset + (hd.scans[2].ecd_end - hd.scans[2].ecd_offset) // 2
    bad = good[:cut] + good[hd.scans[2].ecd_end:]
    with pytest.raises(ValueError) as e:
        jh.decode_batch([good, bad, good], allow_restart=True, allow_progressive=True)
    assert 'damaged JPEG data in file(s) [1]' in str(e.value) and 'status' in str(e.value)
    assert jh.JPEG_STATUS_BITS[1024] == 'end-of-band run beyond the blocks of the scan'
    f = next(f for f in cases.damaged_files() if 'longrun' in f.name)
    assert host[f.name].status[0] & 1024


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_illegal_scripts_and_a_short_workspace_are_refused_before_any_launch(dev):
    f = next(f for f in cases.golden_files() if f.name == 'g_smooth_8x8_q50_444|0|std')
    rows = cases.dpref_rows(f.script)
    edits = [(1, 3, 1), (5, 4, 0), (1, 1, 0), (1, 0, 3), (2, 2, 5), (9, 3, 0), (0, 0, 3), (4, 5, 2), (9, 5, 2)]       # (scan, column, value)
    for s, c, v in edits:
        bad = rows.copy()
        bad[s, c] = v
        coef, status, rounds = _decode([f], 0, dev, script_rows=bad, expect=ERR_ARG)
        assert all((t.view(np.uint8) == FILL).all() for t in (coef, status, rounds)), (s, c, v)
    for short in (1, 4096):
        coef, status, rounds = _decode([f], 0, dev, short=short, expect=ERR_ARG)
        assert all((t.view(np.uint8) == FILL).all() for t in (coef, status, rounds)), short
    with pytest.raises(RuntimeError, match='script'):
        ops.jpeg_decode_progressive(torch.zeros(4, dtype=torch.uint8, device=dev), torch.zeros(2, dtype=torch.int64, device=dev),
                                    torch.zeros((1, 1, 3, 272), dtype=torch.uint8, device=dev), np.zeros((1, 5), np.int32), 8, 8)


def test_without_the_keyword_no_device_is_touched(dev, calls, monkeypatch):
    data = pc.golden()['g_smooth_8x8_q50_444'][0]
    monkeypatch.setattr(jh, 'default_device', lambda: pytest.fail('a device was asked for'))
    del calls[:]
    for fn in (jh.decode_batch, jh.decode_coefficients, jh.transcode_batch):
        with pytest.raises(ValueError) as e:
            fn([data])
        assert str(e.value) == 'progressive file (SOF2): only baseline sequential files (SOF0) are read'
    assert calls == []
