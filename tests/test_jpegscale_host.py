"""Scaled JPEG decoding on the host (no GPU): the restatement (tests/jpegscale_ref.py) against the pixels Pillow
decodes after Image.draft() - every golden case at every scale it can be asked for -, the progressive and restart-interval files of a
case against the same coefficients, the scaled geometry against hand-written values, jpeg_helpers' draft_scale against Pillow's recorded
choices, scaled_size, the refusal of a bad scale, and the sequential core (csrc/jpegscale.h) built into a stand-alone program under
AddressSanitizer and UBSan against the restatement on every case."""
import importlib.util
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

import jpegdprog_ref as dpref
import jpeggrey_ref as gref
import jpegrst_ref as rref
import jpegscale_cases as cases
import jpegscale_ref as sref
from neural_imaging_amd import ops
from neural_imaging_amd.compression import jpeg_helpers as jh


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', cases.CASES, ids=cases.IDS)
def test_restatement_equals_pillow(case):
    g = cases.golden()[0][case.name]
    asked = [s for s in cases.SCALES if cases.askable(case, s)]
    assert sorted(g.crcs) == asked and sorted(g.pixels) == [s for s in asked if cases.pixels_held(case, s)]
    for s in asked:
        got = cases.expected(case, s)
        assert got.shape == sref.scaled_size(case.h, case.w, s) + (1 if case.sampling == 'L' else 3,)
        assert cases.crc(got) == g.crcs[s], (case.name, s)
        if s in g.pixels:
            assert np.array_equal(got, g.pixels[s]), (case.name, s)
    assert g.files['plain'] == cases.restated_file(case)            # so the restatement's coefficients are the file's


def test_no_case_is_left_out():
    g = cases.golden()[0]
    assert sorted(g) == sorted(cases.IDS) and len(set(cases.IDS)) == len(cases.IDS)
    assert {(c.h, c.w) for c in cases.CASES} == set(cases.SIZES) | {cases.BIG}
    for size in cases.SIZES:
        assert {c.sampling for c in cases.CASES if (c.h, c.w) == size} == set(cases.SAMPLINGS)
    for sampling in cases.SAMPLINGS:
        full = [c for c in cases.CASES if (c.h, c.w) == cases.FULL and c.sampling == sampling]
        assert {(c.quality, c.content) for c in full} == {(q, c) for q in cases.QUALITIES for c in cases.CONTENTS}
        assert [c.variants for c in cases.CASES if (c.h, c.w) == cases.VARIED and c.sampling == sampling] == [('plain', 'prog', 'rst')]
    assert {c.quality for c in cases.CASES} == set(cases.QUALITIES) and {c.content for c in cases.CASES} == set(cases.CONTENTS)
    # both sides of the width at which the 4:2:2 up-sampling changes, at every scale, and the widths above it at 1/8
    widths = {c.w for c in cases.CASES if c.sampling == '4:2:2'}
    assert {8, 9, 16, 17, 32, 33, 40, 53, 80} <= widths
    for s in cases.REDUCED:
        ups = {w: sref.geometry(16, w, 2, 1, s)[0][1][3] for w in (4 * s, 4 * s + 1)}
        assert ups == {4 * s: 'replicate', 4 * s + 1: 'fancy' if s < 8 else 'replicate'}
    assert all(sref.geometry(16, w, 2, 1, 8)[0][1][2:] == (-(-w // 16), 'replicate') for w in (33, 40, 53, 80))
    assert all(not cases.askable(c, 8) for c in cases.TINY)


def test_golden_file_is_pillows():
    pytest.importorskip('PIL.Image')
    spec = importlib.util.spec_from_file_location('make_jpegscale_golden', os.path.join(os.path.dirname(cases.GOLDEN), 'make_jpegscale_golden.py'))
    make = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(make)
    g = cases.golden()[0]
    for case in cases.CASES:
        for variant in case.variants:
            data = make.write(case, variant)
            assert data == g[case.name].files[variant], (case.name, variant)
            for s in cases.SCALES:
                if cases.askable(case, s):
                    scale, px = make.draft(data, cases.request(case, s))
                    assert scale == s and cases.crc(px) == g[case.name].crcs[s], (case.name, variant, s)
    assert os.path.getsize(cases.GOLDEN) < 184009


@pytest.mark.parametrize('case', [c for c in cases.CASES if len(c.variants) > 1], ids=lambda c: c.name)
def test_variants_hold_the_same_coefficients(case):
    files, want = cases.golden()[0][case.name].files, cases.flat_coefficients(case)
    assert files['prog'] != files['plain'] != files['rst'] and b'\xff\xc2' in files['prog'] and b'\xff\xdd' in files['rst']
    if case.sampling == 'L':
        flat, status, _ = gref.decode_progressive(files['prog'])
        assert status == 0 and np.array_equal(flat, want)
        assert np.array_equal(gref.decode_baseline(files['rst']).reshape(-1), want)
    else:
        flat, status, _ = dpref.decode(files['prog'])
        assert status == 0 and np.array_equal(flat, want)
        parsed = rref.parse(files['rst'])
        assert parsed['ri'] == cases.RESTART_BLOCKS and np.array_equal(np.concatenate([c.reshape(-1) for c in parsed['coefs']]), want)


# ---- 2. geometry and helpers ----------------------------------------------------------------------------------------------------
# 20 x 27, per sampling and scale: the components' (N, rows, cols, up-sampling) and the output, written out by hand
GEOMETRY_20x27 = {
    ('4:4:4', 1): ([(8, 20, 27, 'none')] * 3, (20, 27)),
    ('4:4:4', 2): ([(4, 10, 14, 'none')] * 3, (10, 14)),
    ('4:4:4', 4): ([(2, 5, 7, 'none')] * 3, (5, 7)),
    ('4:4:4', 8): ([(1, 3, 4, 'none')] * 3, (3, 4)),
    ('4:2:2', 1): ([(8, 20, 27, 'none')] + [(8, 20, 14, 'full')] * 2, (20, 27)),
    ('4:2:2', 2): ([(4, 10, 14, 'none')] + [(4, 10, 7, 'fancy')] * 2, (10, 14)),
    ('4:2:2', 4): ([(2, 5, 7, 'none')] + [(2, 5, 4, 'fancy')] * 2, (5, 7)),
    ('4:2:2', 8): ([(1, 3, 4, 'none')] + [(1, 3, 2, 'replicate')] * 2, (3, 4)),
    ('4:2:0', 1): ([(8, 20, 27, 'none')] + [(8, 10, 14, 'full')] * 2, (20, 27)),
    ('4:2:0', 2): ([(4, 10, 14, 'none')] + [(8, 10, 14, 'none')] * 2, (10, 14)),
    ('4:2:0', 4): ([(2, 5, 7, 'none')] + [(4, 5, 7, 'none')] * 2, (5, 7)),
    ('4:2:0', 8): ([(1, 3, 4, 'none')] + [(2, 3, 4, 'none')] * 2, (3, 4)),
    ('L', 1): ([(8, 20, 27, 'none')], (20, 27)),
    ('L', 2): ([(4, 10, 14, 'none')], (10, 14)),
    ('L', 4): ([(2, 5, 7, 'none')], (5, 7)),
    ('L', 8): ([(1, 3, 4, 'none')], (3, 4)),
}


@pytest.mark.parametrize('sampling,s', list(GEOMETRY_20x27), ids=lambda v: str(v).replace(':', ''))
def test_geometry_20x27(sampling, s):
    hs, vs = (1, 1) if sampling == 'L' else sref.ref.SUBSAMPLING[sampling]
    assert sref.geometry(20, 27, hs, vs, s, 1 if sampling == 'L' else 3) == GEOMETRY_20x27[(sampling, s)]
    assert jh.scaled_size(20, 27, s) == GEOMETRY_20x27[(sampling, s)][1] == ops.jpeg_scaled_size(20, 27, s)
    if sampling == 'L':                                    # whatever factors a one-component file declares
        assert sref.geometry(20, 27, 2, 2, s, 1) == GEOMETRY_20x27[(sampling, s)]


def test_scaled_size():
    assert [jh.scaled_size(h, w, s) for h, w, s in ((1, 1, 8), (8, 9, 8), (17, 16, 2), (4096, 4095, 4), (5, 3, 1))] == \
        [(1, 1), (1, 2), (9, 8), (1024, 1024), (5, 3)]


def test_draft_scale_is_pillows_choice():
    draft = cases.golden()[1]
    assert len(draft) >= 50 and set(draft[:, 4].tolist()) == {1, 2, 4, 8}
    for h, w, rw, rh, scale in draft.tolist():
        assert jh.draft_scale(h, w, (rw, rh)) == scale, (h, w, rw, rh)
    recorded = {tuple(r[:4]): r[4] for r in draft.tolist()}
    assert all(req in recorded for req in cases.DRAFT_REQUESTS)
    assert [recorded[r] for r in ((64, 40, 5, 5), (64, 40, 30, 30), (64, 40, 41, 64), (136, 136, 17, 17), (136, 136, 18, 17))] == [8, 1, 1, 8, 4]


@pytest.mark.parametrize('scale', (0, 3, 16, '2'), ids=str)
def test_bad_scale_is_a_value_error(scale, monkeypatch):
    def never(*a, **k):
        raise AssertionError('a refused scale got as far as the device')
    monkeypatch.setattr(jh, '_decode_groups', never)
    data = cases.golden()[0][cases.IDS[0]].files['plain']
    with pytest.raises(ValueError, match='scale: one of the integers 1, 2, 4, 8 needed'):
        jh.decode_batch([data], scale=scale)
    with pytest.raises(ValueError, match='scale: one of the integers 1, 2, 4, 8 needed'):
        ops.jpeg_reconstruct_scaled(None, 8, 8, None, scale)
    with pytest.raises(ValueError):
        jh.scaled_size(8, 8, scale)


# ---- 3. the sequential core under sanitizers ----------------------------------------------------------------------------------------
def test_host_program_runs_clean():
    images, done = cases.host_reference()
    assert done.returncode == 0 and done.stderr == b'' and done.stdout == b''
    assert len(images) == len(cases.host_jobs()) == 3 * (len(cases.CASES) + len(cases.TINY)) + 3 * len(cases.SAMPLINGS)


@pytest.mark.parametrize('case', cases.CASES + cases.TINY, ids=lambda c: c.name)
def test_host_program_equals_restatement(case):
    images, _ = cases.host_reference()
    for s in cases.REDUCED:
        got = images[cases.Job((case,), s)]
        assert got.shape[0] == 1 and np.array_equal(got[0], cases.expected(case, s)), (case.name, s)


@pytest.mark.parametrize('sampling', cases.SAMPLINGS, ids=lambda v: v.replace(':', ''))
def test_host_program_batch_of_five(sampling):
    images, _ = cases.host_reference()
    five = cases.batch_of_five(sampling)
    assert len(five) == 5
    for s in cases.REDUCED:
        assert np.array_equal(images[cases.Job(five, s)], np.stack([cases.expected(c, s) for c in five])), (sampling, s)


@pytest.mark.parametrize('head', ((1, 8, 8, 1, 1, 3, 1), (1, 8, 8, 1, 1, 3, 3), (1, 8, 8, 1, 1, 3, 16), (1, 8, 8, 1, 2, 3, 2), (1, 8, 8, 2, 2, 1, 2),
                                  (0, 8, 8, 1, 1, 3, 2)), ids=str)
def test_host_program_refuses(head):
    """Scale 1 is not the scaled core's (the full-size reconstruction serves it); other scales, factors and an empty batch are refused."""
    with tempfile.TemporaryDirectory(prefix='jpegscale_refuse_') as work:
        with open(os.path.join(work, 'in.bin'), 'wb') as f:
            f.write(struct.pack('<I7i', 1, *head))
        done = subprocess.run([cases.host_program(), os.path.join(work, 'in.bin'), os.path.join(work, 'out.bin')], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE)
    assert done.returncode == 3 and done.stderr == b''
