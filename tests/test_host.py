"""CPU tests of the product's host side: track pipeline vs the reference's golden
tables, loader error behaviour, and the C-ABI library exports."""
import ctypes
import os
import re

import numpy as np
import pytest

import track_gen
from golden_replay import GOLDEN, TRACKS
from nascargymnasium_amd.track import build_walls, load_track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(f[:-6] for f in os.listdir(TRACKS) if f.endswith(".track"))


@pytest.mark.parametrize("name", NAMES)
def test_python_track_pipeline_bit_exact(name):
    g = np.load(os.path.join(GOLDEN, "tracks.npz"))
    t = load_track(os.path.join(TRACKS, name + ".track"))
    assert np.array_equal(t.segment_table(), g[f"{name}__segments"])
    assert t.total_length == float(g[f"{name}__total_length"])
    assert np.array_equal(build_walls(t), g[f"{name}__walls"])


@pytest.mark.parametrize("name", track_gen.FAMILY)
def test_generated_track_pipeline_bit_exact(name, tmp_path):
    """tests/track_gen.py reproduces the texts stored in tracks_generated.npz, and track.py's tables of them equal the
    reference's own (up to 64 segments, zero-length chords, dropped walls, no start line) bit for bit"""
    g = np.load(os.path.join(GOLDEN, "tracks_generated.npz"))
    assert track_gen.text(name) == str(g[f"{name}__text"])
    t = load_track(track_gen.write(tmp_path, name))
    assert len(t.segments) == track_gen.SEGMENTS[name]
    assert np.array_equal(t.segment_table(), g[f"{name}__segments"])
    assert t.total_length == float(g[f"{name}__total_length"])
    walls = build_walls(t)
    assert walls.shape == g[f"{name}__walls"].shape and len(walls) <= track_gen.MAX_WALLS
    assert np.array_equal(walls, g[f"{name}__walls"])
    assert np.array_equal(np.array(t.start_position, np.float64), g[f"{name}__start_position"])


def test_loader_errors(tmp_path):
    with pytest.raises(FileNotFoundError):
        load_track(str(tmp_path / "missing.track"))
    p = tmp_path / "bad.track"
    p.write_text("WIDTH 12\nGRID\nZIGZAG 3\n")
    with pytest.raises(ValueError, match="Unknown command"):
        load_track(str(p))
    p.write_text("GRID\nLEFT 400 100\n")
    with pytest.raises(ValueError, match="Curve angle"):
        load_track(str(p))
    # non-numeric arguments: Python's own float() message, as the reference re-raises it (its "invalid literal"
    # re-wrap never matches a float() error; src/track_generator.py:370-374, 396-400); upper-cased like the line
    p.write_text("GRID\nSTRAIGHT ten\n")
    with pytest.raises(ValueError, match=r"^could not convert string to float: 'TEN'$"):
        load_track(str(p))
    p.write_text("GRID\nRIGHT 90 wide 3\n")
    with pytest.raises(ValueError, match=r"^could not convert string to float: 'WIDE'$"):
        load_track(str(p))
    p.write_text("GRID\nSTRAIGHT 100 60\n")
    with pytest.raises(ValueError, match="Banking angle must be between -45 and 45 degrees: 60.0"):
        load_track(str(p))
    p.write_text("grid  # comment\nstartline\nstraight 10 5 # banked\n")
    t = load_track(str(p))
    assert [s.segment_type for s in t.segments] == ["GRID", "STARTLINE", "STRAIGHT"]
    assert t.segments[2].banking_angle == 5.0


def test_capi_library_exports_every_declared_symbol():
    from nascargymnasium_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    hdr = open(os.path.join(ROOT, "include", "nascar.h")).read()
    declared = set(re.findall(r"\b(nascar_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTED)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for sym in declared:
        assert hasattr(L, sym), sym


def test_product_library_reads_no_ab_knobs():
    """The product build reads no environment variable that changes a kernel path (round-4 verdict item 7): the A/B
    knobs (NASCAR_EPB, NASCAR_RAY_LPC, NASCAR_FUSE_ML, NASCAR_RBLOCK, NASCAR_BEAM_CELL, NASCAR_SENSOR,
    NASCAR_NO_MAP_SHORTCUT, NASCAR_ACTOR_FP32_VALU) exist only in tools builds (-DNASCAR_AB_KNOBS, tools/mklib.sh);
    the library's only environment reads are GPU_MAX_HW_QUEUES (the process's hardware queues, which bound the
    rollout's shard streams) and NASCAR_VERBOSE (diagnostic prints)."""
    from nascargymnasium_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(m.decode() for m in re.findall(rb"NASCAR_[A-Z0-9_]+", blob))
    assert names <= {"NASCAR_VERBOSE"}, names
