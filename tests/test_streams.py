"""Streams, without a GPU: the table of the side-stream cases (tests/stream_cases.py) against the five headers.  A new entry with a
kbe_stream_t cannot arrive without a case, no case names an entry the headers do not declare, and the bars are the ones the suite already has."""
import ast
import os

import numpy as np
import pytest

import stream_cases as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_reader_finds_the_declarations_with_a_stream():
    entries = sc.stream_entries()
    assert len(entries) == len(set(entries)) == 41
    assert entries[:3] == ['kbe_selftest_err', 'kbe_selftest_division', 'kbe_zkeys_clear'] and entries[-1] == 'kbe_dof_u8'
    assert 'kbe_render_video' in entries and 'kbe_gif_lut' in entries and 'kbe_area_reduce_u8' in entries and 'kbe_crop_area_u8' in entries
    # what takes no stream is no entry of the table: size functions, the ABI numbers, the hand-off's status
    assert not {'kbe_frame_scratch_bytes', 'kbe_abi_version', 'kbe_video_handoff_status', 'kbe_render_frame_group_ahead_ok', 'kbe_gif_bound'} & set(entries)


def test_the_reader_agrees_with_the_bindings_prototypes():
    """The same declarations as the ctypes binding reads from the headers (_cabi.prototypes): those with a c_void_p named kbe_stream_t."""
    from ken_burns_effect_amd import _cabi
    for header, api in (('kbe.h', 'KBE_API'), ('kbe_gif.h', 'KBE_GIF_API'), ('kbe_area.h', 'KBE_AREA_API'), ('kbe_crop_area.h', 'KBE_CROP_AREA_API'), ('kbe_dof.h', 'KBE_DOF_API')):
        with open(os.path.join(sc.ROOT, 'include', header)) as f:
            text = f.read()
        assert set(sc.stream_entries((header,))) <= set(_cabi.prototypes(text, api)), header
        assert sc.stream_entries((header,)), header


def test_every_declaration_with_a_stream_has_a_case():
    covered = {e for c in sc.CASES for e in c.entries}
    assert not set(sc.stream_entries()) - covered, 'declarations with a kbe_stream_t that no side-stream case calls: %s' % sorted(set(sc.stream_entries()) - covered)


@pytest.mark.parametrize('entry', sc.stream_entries())
def test_an_entry_without_its_rows_is_missed(entry):
    """The coverage check can fail: without the rows that name an entry, that entry is reported."""
    covered = {e for c in sc.CASES if entry not in c.entries for e in c.entries}
    assert entry not in covered and any(entry in c.entries for c in sc.CASES)


def test_no_case_names_an_entry_the_headers_do_not_declare():
    declared = set(sc.stream_entries())
    for c in sc.CASES:
        assert c.entries and set(c.entries) <= declared, (c.name, set(c.entries) - declared)


def test_the_tables_rows_are_well_formed():
    assert len({(c.group, c.name) for c in sc.CASES}) == len(sc.CASES)
    # (the rows per group, so that none leaves unnoticed: 33 thunks and two self-tests; 3; 10 on each of two rasters; 9 on each of two sizes and two routes; 6 + 5; 6)
    assert {g: len(sc.cases_of(g)) for g in ('glue', 'abi', 'frame', 'video', 'units', 'python')} == {'glue': 35, 'abi': 3, 'frame': 20, 'video': 36, 'units': 11, 'python': 6}
    assert {c.group for c in sc.CASES} == {'glue', 'abi', 'frame', 'video', 'units', 'python'}
    for c in sc.CASES:
        assert all(name in sc.BARS for name in c.bar.split(' / ')), c
        assert c.synchronises is None or c.group == 'python', 'only tensor-level calls that synchronise by contract run without the query() condition'
    assert [c.name for c in sc.CASES if c.synchronises] == ['render_frames delivered', 'render_frames out_size', 'render_frames lens', 'write_gif', 'mjpeg_encode']


def test_the_bars_are_the_suites_own():
    """Bit for bit; the float-atomic entries' bound; DESIGN section 2's bar for frames -- on arrays that sit on either side of each."""
    a = np.array([0.0, 1.0, 100.0], np.float32)
    sc.check([a], [a.copy()], 'bits', '')
    with pytest.raises(AssertionError):
        sc.check([a], [np.nextafter(a, np.float32(200))], 'bits', '')
    with pytest.raises(AssertionError):
        sc.check([np.array([0.0, -0.0], np.float32)], [np.array([0.0, 0.0], np.float32)], 'bits', '')
    sc.check([a * np.float32(1 + 1e-5)], [a], 'atomic', '')
    with pytest.raises(AssertionError):
        sc.check([a * np.float32(1 + 4e-5)], [a], 'atomic', '')
    with pytest.raises(AssertionError):
        sc.check([a + np.float32(1e-7)], [a], 'atomic', '')                  # a pixel touched that the other left at 0
    frame = np.full(20000, 100, np.uint8)
    few, many, far = frame.copy(), frame.copy(), frame.copy()
    few[:19] += 1
    many[:21] += 1
    far[0] += 2
    sc.check([few], [frame], 'frames', '')
    for wrong in (many, far):
        with pytest.raises(AssertionError):
            sc.check([wrong], [frame], 'frames', '')
    assert sc.differing([many], [frame], 'frames') == [0.0] and sc.differing([far], [frame], 'frames') == [1 / 20000]
    assert sc.differing([np.zeros(3, np.uint8)], [np.zeros(5, np.uint8)], 'bits') == [0.4]
    assert sc.bars_of('frames', 3) == ['frames'] * 3 and sc.bars_of(sc.ONE_FRAME, 5)[1:3] == ['bits', 'bits']


def test_the_gpu_module_runs_every_row_of_the_table():
    """tests/test_streams_gpu.py takes its cases from the table: each group is asked for by name there, and the glue thunks' shapes are the table's."""
    with open(os.path.join(HERE, 'test_streams_gpu.py')) as f:
        tree = ast.parse(f.read())
    asked = {n.args[0].value for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, 'id', getattr(n.func, 'attr', '')) in ('ids', 'cases_of')
             and n.args and isinstance(n.args[0], ast.Constant)}
    assert asked == {c.group for c in sc.CASES}, asked
    assert set(sc.VECTOR_THUNKS) <= set(sc.GLUE) and len(sc.GLUE) == 35
