"""TEST INFRASTRUCTURE ONLY: the picture sizes of the edge-geometry sweep (tests/test_geom_sweep_cpu.py, tests/test_gpu_geom_sweep.py),
one list per feature library, BUILT from that library's tile constants -- read from the emulated-kernel libraries, which compile the
kernel headers themselves (ve_tile, ae_tile, me_tile, se_tile, ce_tile, xe_band / xe_block), and from the geometry functions the
*_util helpers already use.  A tile size that changes in a kernel header changes these lists.

For a tile T (x) by U (y), in the unit the kernel tiles in (pixels of a scale for VIF, band pixels for ADM, ...), and each scale s of
the library's pyramid, a size is made whose scale-s dimension is each of EDGES: T - 1, T, T + 1, 2 T - 1, 2 T + 1 and T + r for r = 1,
2, 3 (the remainders of the 4-sample groups).  The scale-0 dimension is the SMALLEST n not below the library's minimum whose scale-s
dimension -- as the library's own geometry function reports it: n >> s for VIF, the halvings that round up of ADM and CAMBI -- is the
target; a target that no allowed n has (a 15-row picture for a library that starts at 32) is left out.  n + 1 is added wherever it has
the same scale-s dimension (the `odd` variant: a remainder appears at the scales above s, rows there end in padding).

Widths and heights are not crossed: every edge width is paired with a plain height and with one edge height (_pairs says which), and
the reverse.  Every list is a dict {(w, h): [(axis, scale, edge), ...]} in the order built: iterating it gives the sizes, its values say
which edges a size stands for.  `coverage` says which edges ANY list of sizes reaches, and `fixed_sizes` holds the hand-picked sizes the
libraries' own tests had before the sweep: tests/test_geom_sweep_cpu.py holds the gap they left to the table in docs/LABBOOK.md.

`assign(sizes, n_cases, n_kinds)` is the rotation both tiers use.  Rotating the layout by the plain list index leaves holes, because
the lists are periodic themselves (ADM's x T+1 would meet 7 of 8 layouts, and with 8 layouts `index % 2` is the layout's own parity), so
the index that picks the layout and the alternation bit (aligned or not, wide loads or not) is the entry's RANK AMONG THE ENTRIES OF ITS
OWN (axis, edge): every x edge then meets every layout, and every layout both values of the bit, within 16 of its entries.
tests/test_geom_sweep_cpu.py asserts what that reaches."""
import ctypes as C
from functools import lru_cache

from tests import adm_util, cambi_util, motion_util, scene_util, vif_util, xpsnr_util

EDGES = (("T-1", lambda T: T - 1), ("T", lambda T: T), ("T+1", lambda T: T + 1), ("2T-1", lambda T: 2 * T - 1), ("2T+1", lambda T: 2 * T + 1),
         ("T+2", lambda T: T + 2), ("T+3", lambda T: T + 3))
DROPPABLE = ("2T-1", "2T+1")  # and any `odd` variant; never another edge


def deep_doubles_and_odd(t):
    """what the GPU tier's thinning rule lets go (`drop=`): 2T-1 / 2T+1 at scales >= 2, and the odd variants"""
    return t[2].endswith(" odd") or t[1] >= 2


def edge_of(tag):
    """(axis, edge) of a tag, an odd variant counted with its edge"""
    return tag[0], tag[2].replace(" odd", "")


def assign(sizes, n_cases, n_kinds):
    """[(w, h, tags, case index, kind index, bit, bit2)], one per size in order.  j is the entry's rank among the entries whose first
    tag has the same (axis, edge).  The case cycles with j and starts one earlier every full turn, the bit is j's parity: the first and
    the last case of the list (y8 and the packed layout, the two with load paths of their own) meet both values of the bit within ten
    entries of an edge, every case within sixteen.  The kind cycles with the list index, which the ranks are not tied to; bit2 (CAMBI's
    default window) changes every second entry of the list."""
    rank, out = {}, []
    for i, ((w, h), tags) in enumerate(sizes.items()):
        j = rank.get(edge_of(tags[0]), 0)
        rank[edge_of(tags[0])] = j + 1
        out.append((w, h, tags, (j - j // n_cases) % n_cases, i % n_kinds, j % 2, i // 2 % 2))
    return out


def _consts(build, fn, n, typ=C.c_int):
    out = (typ * n)()
    getattr(C.CDLL(build()), fn)(out)
    return [int(v) for v in out]


def _smallest(dim, target, s, minimum):
    """the smallest n >= minimum with dim(n, s) == target (dim does not decrease with n), or None"""
    n = minimum
    while True:
        d = dim(n, s)
        if d >= target:
            return n if d == target else None
        n += 1


def _axis(dim, T, scales, minimum):
    """[(n, scale, edge)] of one axis"""
    out = []
    for s in scales:
        for name, f in EDGES:
            n = _smallest(dim, f(T), s, minimum)
            if n is None:
                continue
            out.append((n, s, name))
            if dim(n + 1, s) == f(T):
                out.append((n + 1, s, name + " odd"))
    return out


PARTNER_SCALE = 1  # see _pairs


def _pairs(ws, hs, plain_w, plain_h, extras=(), drop=None):
    """{(w, h): tags}: every edge width with the plain height and one edge height, every edge height with the plain width
    and one edge width, then the extras [(w, h, tag)]; de-duplicated, first occurrence kept.  The edge partner of a scale-s entry is
    taken, in turn, from the edges of scale min(s, PARTNER_SCALE) of the other axis: an entry of scale 0 or 1 meets edges of its own
    scale, and the entries of the deep scales -- several hundred to two thousand samples long -- stay strips a few tiles across
    instead of pictures of a quarter megapixel, which is what keeps the restatements affordable."""
    tags = {}

    def add(w, h, *t):
        tags.setdefault((w, h), [])
        tags[(w, h)] += [x for x in t if x not in tags[(w, h)]]
    for i, (w, s, e) in enumerate(ws):
        same = [x for x in hs if x[1] == min(s, PARTNER_SCALE)] or hs
        h2, s2, e2 = same[i % len(same)]
        add(w, plain_h, ("x", s, e))
        add(w, h2, ("x", s, e), ("y", s2, e2))
    for i, (h, s, e) in enumerate(hs):
        same = [x for x in ws if x[1] == min(s, PARTNER_SCALE)] or ws
        w2, s2, e2 = same[i % len(same)]
        add(plain_w, h, ("y", s, e))
        add(w2, h, ("x", s2, e2), ("y", s, e))
    for w, h, t in extras:
        add(w, h, t)
    if drop is not None:
        may_go = lambda t: (t[2].endswith(" odd") or t[2] in DROPPABLE) and drop(t)
        tags = {k: v for k, v in tags.items() if not all(may_go(t) for t in v)}
    return tags


def coverage(sizes, dim_w, dim_h, T, U, scales):
    """the set of (axis, scale, edge) that `sizes` reach: a scale-s dimension equal to an edge value of the tile"""
    got = set()
    for w, h in sizes:
        for axis, n, dim, t in (("x", w, dim_w, T), ("y", h, dim_h, U)):
            for s in scales:
                got |= {(axis, s, e) for e, f in EDGES if dim(n, s) == f(t)}
    return got


# ---- VIF: 48 x 16 pixels of each of four scales, n >> s ---------------------------------------------------------------------------
@lru_cache(None)
def _vif_dims(n):
    ws, hs = (C.c_int * 4)(), (C.c_int * 4)()
    assert vif_util.emul_lib().ve_sizes(n, 32, 0, 8, ws, hs) == 0
    return tuple(ws)


def vif_dim(n, s):
    return _vif_dims(n)[s]


def vif_tile():
    return _consts(vif_util.build_emul, "ve_tile", 2)


def vif(drop=None):
    T, U = vif_tile()
    return _pairs(_axis(vif_dim, T, range(4), 32), _axis(vif_dim, U, range(4), 32), 37, 37, drop=drop)


# ---- ADM: 32 x 16 band pixels of each of four scales; a band is half its source, rounded up -------------------------------------------
@lru_cache(None)
def _adm_dims(n):
    return tuple(x[2] for x in adm_util.geom(n, 32)["sizes"])


def adm_dim(n, s):
    return _adm_dims(n)[s]


def adm_tile():
    return _consts(adm_util.build_emul, "ae_tile", 2)


def adm(drop=None):
    T, U = adm_tile()
    return _pairs(_axis(adm_dim, T, range(4), 32), _axis(adm_dim, U, range(4), 32), 37, 37, drop=drop)


# ---- motion: 120 x 16 pixels, one scale; and pictures smaller than the 5-tap blur reaches ---------------------------------------------
def one_scale(n, s):
    return n


def motion_tile():
    return _consts(motion_util.build_emul, "me_tile", 2)


def motion(drop=None):
    T, U = motion_tile()
    tiny = [(w, h, ("tiny", 0, "below the blur's reach")) for w in (3, 4, 5, 7) for h in (3, 4, 5)]
    return _pairs(_axis(one_scale, T, (0,), 3), _axis(one_scale, U, (0,), 3), 9, 9, tiny, drop)


# ---- scene: one pass of the lanes is 4 x 256 samples of a row, 8 rows in flight; bands of about 65536 samples, at most 128 rows ----------
def scene_consts():
    band_samples, rows, rows_max, lane_pass = _consts(scene_util.build_emul, "se_tile", 4, C.c_uint)
    return band_samples, rows, rows_max, lane_pass


def scene_band_rows(w):
    band_samples, _, rows_max, _ = scene_consts()
    return max(1, min(rows_max, band_samples // w))


def scene(drop=None):
    band_samples, rows, rows_max, lane_pass = scene_consts()
    extras = []
    # either side of one band: a width whose band is the most rows a band may have, the first width whose band is one row less, and
    # the width just past one pass of the lanes
    for w in (band_samples // rows_max, band_samples // rows_max + 1, lane_pass + 1):
        br = scene_band_rows(w)
        assert scene_util.bands(w, br, "y8", 8) == 1 and scene_util.bands(w, br + 1, "y8", 8) == 2
        extras += [(w, h, ("band", 0, f"{br} rows {h - br:+d}")) for h in (br - 1, br, br + 1, 2 * br + 1)]
    # either side of TMS_BAND_ROWS_MAX where the clamp decides (a narrow picture, whose band would otherwise be the whole of it)
    extras += [(33, h, ("band", 0, f"rows max {h - rows_max:+d}")) for h in (rows_max - 1, rows_max, rows_max + 1)]
    return _pairs(_axis(one_scale, lane_pass, (0,), 1), _axis(one_scale, rows, (0,), 1), 5, 5, extras, drop)


# ---- CAMBI: the mask kernel's 64 x 16 tile, five scales that halve rounding up; strips of TMC_MAX_COLS - 2 pad columns ------------------
@lru_cache(None)
def _cambi_dims(n):
    return tuple(cambi_util.geom(n, 32, "y8", 8, 3).w)


def cambi_dim(n, s):
    return _cambi_dims(n)[s]


def cambi_tile():
    return _consts(cambi_util.build_emul, "ce_tile", 3, C.c_uint)


CAMBI_STRIP_WINDOWS = (3, 15)  # of cambi_util.WINDOWS


def cambi(drop=None):
    """cambi_window(tags of a size, bit) is that size's window"""
    T, U, max_cols = cambi_tile()
    extras = []
    for win in CAMBI_STRIP_WINDOWS:
        assert win in cambi_util.WINDOWS
        oc = cambi_util.geom(64, 64, "y8", 8, win).oc  # columns a workgroup writes: max_cols less the window's reach on either side
        assert oc == max_cols - 2 * (win // 2)
        for s in (0, 1):
            for t in (oc - 1, oc, oc + 1, 2 * oc + 1):
                extras.append((_smallest(cambi_dim, t, s, 32), 37 + 2 * s, ("strip", s, f"window {win} oc {t - oc:+d}" if t <= oc + 1 else f"window {win} 2 oc + 1")))
    return _pairs(_axis(cambi_dim, T, range(5), 32), _axis(cambi_dim, U, range(5), 32), 37, 37, extras, drop)


def cambi_window(tags, bit):
    """the window a strip entry was built for, else one of the two small ones by `bit`"""
    for t in tags:
        if t[0] == "strip":
            return int(t[2].split()[1])
    return (3, 7)[bit]


# ---- XPSNR: blocks of b x b samples, b from the picture (4 (int)(32 sqrt(w h / (3840 2160)) + 0.5)); bands of TMX_BAND rows in a block ----
XPSNR_CASES = (("nv12", 8), ("p016", 10), ("p016", 12), ("p016", 16), ("i420", 8), ("i420", 10), ("i420", 12), ("i420", 16), ("i420p10", 10))


@lru_cache(None)
def _xpsnr_lib():
    return C.CDLL(xpsnr_util.build_emul())


def xpsnr_band():
    return int(_xpsnr_lib().xe_band())


@lru_cache(None)
def xpsnr_block(w, h):
    """the block size of a w x h picture: 0 where the library refuses it, -1 where b < 4 (one block, plain SSE)"""
    return int(_xpsnr_lib().xe_block(w, h, 2, 8))


def xpsnr(drop=None):
    """The tile is the picture's own block (b >= 4 from 43 x 48 samples on), so a picture is never one or two tiles wide and an edge
    is the LAST block: one sample short of whole (T-1), whole (T), or 1, 2, 3 samples (T+1 .. T+3) -- per plain / edge size of the
    other axis, the smallest accepted n with that remainder.  There is no 2T entry.  The band of TMX_BAND rows splits a block only
    where b > TMX_BAND (from about 0.6 megapixels): the last block row of such a picture is given TMX_BAND - 1 .. TMX_BAND + 3 rows."""
    band = xpsnr_band()
    names = {-1: "T-1", 0: "T", 1: "T+1", 2: "T+2", 3: "T+3"}
    extras = []
    for axis, wide in (("x", True), ("y", False)):
        for other in (48, 61):
            for d, e in names.items():
                for n in range(8, 4000):
                    w, h = (n, other) if wide else (other, n)
                    b = xpsnr_block(w, h)
                    if b >= 4 and n % b == d % b:
                        extras.append((w, h, (axis, 0, e)))
                        break
    # the band inside a block: the smallest b above the band, a picture of 14 whole block rows and a last one of band + d rows
    b = band + 4
    for d, e in names.items():
        h = 14 * b + band + d
        w = next(w for w in range(8, 8000, 2) if xpsnr_block(w, h) == b)
        extras.append((w, h, ("band", 0, e)))
    return _pairs([], [], 0, 0, extras, drop)
