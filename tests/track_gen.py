"""Generated `.track` texts of up to 64 segments.  TEST INFRASTRUCTURE, CPU only.

The bundled tracks have 7-9 segments and start at the origin, heading +x, with the start line as segment 1.  This
family is what the track lookups need beyond that (nascar_add_track takes up to MAX_SEG = 64 segments; the logic
kernel's chord screen keeps the first 16 chords in registers and loops over the rest):

  seg17       17 segments: one chord past the screen's registers.  A closed oval; every curve and every piece of the
              back straight carries its own banking.
  seg64       64 segments, 52 of them curves of 12 or 15 degrees (LEFT and RIGHT mixed), each with its own banking in
              [-45, 45], so that a wrong nearest chord shows in `bank`.  The STARTLINE is segment 20, after a curve:
              neither axis-aligned nor at the origin.  Two point-symmetric halves, so the loop closes.
  ring4       four LEFT 90 curves: the chords form a square whose centre is equidistant from all four.  No GRID and no
              STARTLINE.
  nostart     an oval without GRID and STARTLINE: startline = -1, start position (0, 0).
  degenerate  STRAIGHT 0 (the chord's ll == 0), STRAIGHT 0.0005 (ll < 1e-6), STRAIGHT 0.05 (walls shorter than 0.1 m
              are dropped), a LEFT curve with radius < width / 2 (no inner wall: the builder drops the curve's walls),
              a 5-degree curve (the 8-chord minimum), a second STARTLINE (the first counts) and a closing LEFT 360.
  seg1        a single GRID line: one segment, two walls.

text(name) is the file's text; write(directory, name) writes it (asserting the wall count that the sensors' LDS wall
image allows, and the extent) and returns the path, as crowded.write_pocket does.  tests/golden/tracks_generated.npz
holds the texts and the reference's own tables of them (oracle/gen_golden.py).
"""
import os

FAMILY = ("seg1", "ring4", "seg17", "seg64", "nostart", "degenerate")
MAX_WALLS = 3000        # the sensor kernel's wall image must fit in LDS
MAX_EXTENT = 1500.0     # metres: keeps the beam builds at a few seconds


def _seg17():
    L = ["WIDTH 16", "GRID", "STARTLINE", "STRAIGHT 150 3"]
    L += [f"LEFT 45 150 {b}" for b in (10, 12, 14, 16)]
    L += [f"STRAIGHT {n} {b}" for n, b in ((60, -3), (50, -5), (45, -7), (40, -9), (35, -11), (25, -13))]   # 255 m
    L += [f"LEFT 45 150 {b}" for b in (18, 20, 22, 24)]
    return L


def _seg64():
    """two halves of 32 pieces, each turning 180 degrees to the left: 20 LEFT (12 / 15 degrees) and 6 RIGHT 15"""
    straight = {0: 100, 6: 60, 12: 40, 20: 5, 25: 50, 30: 30}
    L = ["WIDTH 16"]
    curve = 0
    for half in range(2):
        j = left = 0
        for k in range(32):
            if k in straight:
                L.append("GRID" if (half, k) == (0, 0) else "STARTLINE" if (half, k) == (0, 20) else f"STRAIGHT {straight[k]}")
                continue
            bank = (curve * 37) % 91 - 45          # 37 and 91 are coprime: 52 distinct values
            if j % 4 == 2 and j < 24:
                L.append(f"RIGHT 15 220 {bank}")
            else:
                L.append(f"LEFT {(12, 15)[left % 2]} {160 + 10 * (left % 5)} {bank}")
                left += 1
            j += 1
            curve += 1
    return L


_LINES = {
    "seg1": ["GRID"],
    "ring4": ["WIDTH 16", "LEFT 90 100 10", "LEFT 90 100 -20", "LEFT 90 100 30", "LEFT 90 100 0.05"],
    "seg17": _seg17(),
    "seg64": _seg64(),
    "nostart": ["WIDTH 14", "STRAIGHT 200", "LEFT 180 80 12", "STRAIGHT 200 2", "LEFT 180 80 -8"],
    "degenerate": ["WIDTH 12", "GRID", "STARTLINE", "STRAIGHT 60", "STRAIGHT 0 7", "LEFT 90 60 15", "STRAIGHT 0.0005 -10",
                   "LEFT 5 100 20", "STRAIGHT 0.05 -4", "LEFT 20 5 -30", "STARTLINE", "STRAIGHT 80 5", "LEFT 65 60",
                   "STRAIGHT 165", "LEFT 90 60 25", "STRAIGHT 100 -2", "LEFT 360 30 9"],
}
SEGMENTS = {"seg1": 1, "ring4": 4, "seg17": 17, "seg64": 64, "nostart": 4, "degenerate": 16}


def text(name):
    return "\n".join(_LINES[name]) + "\n"


def too_many_segments(n=65):
    """a text of n STRAIGHT 10 segments (n = 65: one more than nascar_add_track takes)"""
    return "GRID\n" + "STRAIGHT 10\n" * (n - 1)


def flat(name):
    """track `name` with every banking argument removed (has_banking = 0: the progress-only lookup)"""
    out = []
    for ln in _LINES[name]:
        p = ln.split()
        keep = {"STRAIGHT": 2, "LEFT": 3, "RIGHT": 3}.get(p[0], len(p))
        out.append(" ".join(p[:keep]))
    return "\n".join(out) + "\n"


_checked = set()


def write(directory, name, txt=None):
    """track `name` (or the text `txt` under that name) written under `directory`; returns its path"""
    from nascargymnasium_amd.track import build_walls, load_track
    path = os.path.join(str(directory), name + ".track")
    with open(path, "w") as f:
        f.write(text(name) if txt is None else txt)
    if txt is None and name not in _checked:
        t = load_track(path)
        w = build_walls(t)
        assert len(t.segments) == SEGMENTS[name], (name, len(t.segments))
        assert len(w) <= MAX_WALLS, (name, len(w))
        assert (w[:, :2].max(0) - w[:, :2].min(0)).max() < MAX_EXTENT, (name, w[:, :2].min(0), w[:, :2].max(0))
        _checked.add(name)
    return path
