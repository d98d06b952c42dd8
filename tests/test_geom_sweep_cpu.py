"""No-GPU tier of the edge-geometry sweep: for every feature library, the kernel SOURCE executed lane by lane on the CPU (tests/*_emul)
against the numpy restatement (tests/*_ref.py) at EVERY size of tests/geom_sweep.py -- sizes built from the kernels' tile constants so
that the picture edge falls one short of, on, and just past a tile boundary, at every scale of the pyramids.  The comparison is each
library's own (imported from its test module): the integer / f32 planes of every scale bit-exact where the emulator has a plane hook,
the sums within the tolerance that module derives.  No tolerance is introduced here.

VIF, ADM and CAMBI (and XPSNR at its five large sizes) rotate the layout / depth, the content kind and the memory form (an odd pitch at whatever base numpy gives,
or a 16-byte aligned base and pitch: the wide loads) by geom_sweep.assign, and test_the_rotation_reaches_every_load_path holds what
that reaches; motion, scene and XPSNR's small sizes, which cost little, run EVERY layout at every size.  Every plane has padding past its rows and every
ignorable bit and padding byte is garbage.  A test runs its whole list and then reports every size that failed, not the first.

Sizes and time (the six tests side by side on one machine, one core each; the emulated kernels, 256 host threads per workgroup, are
nearly all of it; of the restatements alone, on a core to itself: vif 4.7 s, adm 1.9 s, cambi 26 s, xpsnr 3 s), as printed by each test:
  vif 171 sizes 101 s, adm 181 sizes 101 s, cambi 215 sizes 314 s, motion 33 sizes x 8 layouts x 3 memory forms 121 s,
  scene 36 sizes x 8 layouts x 2 forms 73 s, xpsnr 21 sizes (16 of them x 9 layouts) 146 s, most of it the five 0.6-megapixel pictures:
  a band splits a block only from there"""
import time

from tests import adm_ref, adm_util, cambi_ref, cambi_util, geom_sweep as G, motion_ref, motion_util, scene_util, vif_ref, vif_util
from tests import test_adm_cpu, test_cambi_cpu, test_motion_cpu, test_scene_cpu, test_vif_cpu, test_xpsnr_cpu
from tests import xpsnr_util

MOTION_KINDS = ("random", "extreme", "smooth")
# what each library's test_emulated_kernel_matches_the_restatement ran before the sweep
FIXED = {"vif": test_vif_cpu.SIZES, "adm": test_adm_cpu.SIZES, "motion": test_motion_cpu.SIZES, "cambi": cambi_util.SIZES}


def libraries():
    """(name, list, scale-s dimension, (T, U), scales, minimum) of the libraries whose tiles are fixed"""
    return (("vif", G.vif(), G.vif_dim, G.vif_tile(), range(4), 32), ("adm", G.adm(), G.adm_dim, G.adm_tile(), range(4), 32),
            ("motion", G.motion(), G.one_scale, G.motion_tile(), (0,), 3), ("cambi", G.cambi(), G.cambi_dim, G.cambi_tile()[:2], range(5), 32))


def sweep(name, entries, one, t0=None):
    """one(*entry) for EVERY entry; the failures are collected and reported together"""
    t0, failed = t0 or time.time(), []
    for e in entries:
        try:
            one(*e)
        except AssertionError as x:
            failed.append(f"{e[0]}x{e[1]}: {str(x)[:300]}")
    print(f"{name}: {len(entries)} sizes, {time.time() - t0:.1f} s")
    assert not failed, f"{name}: {len(failed)} of {len(entries)} sizes differ:\n" + "\n".join(failed)


def wide(U, layout, Y, bits, dirty):
    """the plane at a 16-byte aligned base and pitch with garbage in the padding (the wide loads), as tests/test_cambi_cpu.py has it"""
    return cambi_util.aligned_copy(U.luma_plane(layout, Y, bits, dirty=dirty), 3 if layout != "y10_packed" else 0)


def test_the_lists_follow_the_tile_constants():
    """each list holds, at every scale, a size on either side of the tile in both axes -- computed from the constants, not typed in"""
    for name, sizes, dim, (T, U), scales, least in libraries():
        got = G.coverage(sizes, dim, dim, T, U, scales)
        for s in scales:
            for e, f in G.EDGES:
                assert ("x", s, e) in got, (name, s, e)                       # every width edge is above every library's minimum
                assert (("y", s, e) in got) == (G._smallest(dim, f(U), s, least) is not None), (name, s, e)
        assert all(w >= least and h >= least for w, h in sizes) and len(set(sizes)) == len(sizes)
    T = G.vif_tile()[0]
    assert {(T - 1, 37), (T, 37), (T + 1, 37), (T * 8, 37), (T * 8 + 1, 37), ((2 * T + 1) * 8, 37)} <= set(G.vif())
    assert {(w, h) for w in (3, 4, 5, 7) for h in (3, 4, 5)} <= set(G.motion())
    band_samples, rows, rows_max, lane_pass = G.scene_consts()
    assert {(33, rows_max - 1), (33, rows_max), (33, rows_max + 1), (lane_pass - 1, 5), (lane_pass + 1, 5)} <= set(G.scene())
    mc, cambi = G.cambi_tile()[2], G.cambi()
    assert {(mc - 2 - 1, 37), (mc - 2, 37), (mc - 2 + 1, 37), (mc - 14, 37), (mc - 14 + 1, 37)} <= set(cambi)
    assert G.cambi_window(cambi[(mc - 14, 37)], 0) == 15 and G.cambi_window(cambi[(mc - 2, 37)], 1) == 3
    assert G.cambi_window(cambi[(65, 37)], 0) == 3 and G.cambi_window(cambi[(65, 37)], 1) == 7
    assert all(G.xpsnr_block(w, h) >= 4 for w, h in G.xpsnr())


def family(case):
    """the sample loaders (tm_sample_load.h) have one wide-load branch per storage format"""
    return {"y8": "u8", "y10_packed": "packed"}.get(case[0], "u16")


def test_the_rotation_reaches_every_load_path():
    """geom_sweep.assign over the lists as both tiers run them: every layout meets both memory forms, every content kind, and (CAMBI)
    both default windows; at EVERY x edge (the axis the loaders run along) every layout appears and every storage format meets both
    memory forms; in the full lists every (layout, memory form) pair appears at every x edge but at most one."""
    thin = G.cambi(drop=G.deep_doubles_and_odd)
    for name, sizes, cases, kinds, full in (("vif", G.vif(), vif_util.CASES, vif_util.CONTENTS, True), ("adm", G.adm(), adm_util.CASES, adm_util.CONTENTS, True),
                                              ("cambi", G.cambi(), cambi_util.CASES, cambi_util.KINDS, True), ("cambi, thinned", thin, cambi_util.CASES, cambi_util.KINDS, False)):
        got = G.assign(sizes, len(cases), len(kinds))
        assert len(got) == len(sizes)
        assert {(c, b) for _, _, _, c, _, b, _ in got} == {(c, b) for c in range(len(cases)) for b in (0, 1)}, name
        assert {(c, k) for _, _, _, c, k, _, _ in got} == {(c, k) for c in range(len(cases)) for k in range(len(kinds))}, name
        assert {(k, b) for _, _, _, _, k, b, _ in got} == {(k, b) for k in range(len(kinds)) for b in (0, 1)}, name
        if name.startswith("cambi"):
            plain = [g for g in got if not any(t[0] == "strip" for t in g[2])]
            assert {(c, b2) for _, _, _, c, _, _, b2 in plain} == {(c, b2) for c in range(len(cases)) for b2 in (0, 1)}, name
            strips = {t[2]: set() for g in got for t in g[2] if t[0] == "strip"}
            for _, _, tags, c, _, b, _ in got:
                for t in tags:
                    if t[0] == "strip":
                        strips[t[2]].add(b)
            assert len(strips) == 8 and all(v == {0, 1} for v in strips.values()), strips  # either side of a strip, both memory forms
        at = {}
        for _, _, tags, c, _, b, _ in got:
            for t in tags:
                at.setdefault(G.edge_of(t), set()).add((c, b))
        xs = {e: v for e, v in at.items() if e[0] == "x"}
        assert set(xs) == {("x", e) for e, _ in G.EDGES}
        short = 0
        for e, v in xs.items():
            assert {c for c, _ in v} == set(range(len(cases))), (name, e)
            fams = {(family(cases[c]), b) for c, b in v}
            if name == "cambi, thinned" and e == ("x", "T"):  # nine entries are left of this edge: one short of y8's second turn
                assert fams == {(f, b) for f in ("u8", "u16", "packed") for b in (0, 1)} - {("u8", 1)}
                continue
            assert fams == {(f, b) for f in ("u8", "u16", "packed") for b in (0, 1)}, (name, e, fams)
            short += len(v) < 2 * len(cases)
        assert not full or short <= 1, (name, short)
        assert all(len({c for c, _ in v}) >= len(cases) - 2 for e, v in at.items() if e[0] == "y"), name  # a y edge has as few as six entries


def test_the_gap_the_fixed_sizes_left():
    """which (axis, scale, edge) the hand-picked sizes of the libraries' own tests reach -- the table in docs/LABBOOK.md, held here so
    that it stays true -- and that the sweep reaches all of them and every other one that exists"""
    old = {name: G.coverage(FIXED[name], dim, dim, T, U, scales) for name, _, dim, (T, U), scales, _ in libraries()}
    assert old == OLD_COVERAGE, old
    for name, sizes, dim, (T, U), scales, least in libraries():
        new = G.coverage(sizes, dim, dim, T, U, scales)
        exist = {(a, s, e) for a, t in (("x", T), ("y", U)) for s in scales for e, f in G.EDGES if G._smallest(dim, f(t), s, least) is not None}
        assert old[name] <= new and exist <= new, name
        print(name, "fixed sizes", len(old[name]), "of", len(exist), "sweep", len(new & exist))
    # scene's tile is one pass of the lanes by the rows in flight, XPSNR's the picture's own block: the fixed sizes and the edges
    _, rows, _, lane_pass = G.scene_consts()
    assert G.coverage(test_scene_cpu.SIZES, G.one_scale, G.one_scale, lane_pass, rows, (0,)) == OLD_SCENE


OLD_COVERAGE = {"vif": {("x", 1, "T+2"), ("y", 1, "T"), ("y", 1, "T+1")},
                "adm": {("x", 1, "T+1"), ("y", 0, "T"), ("y", 0, "T+2"), ("y", 1, "T+2")},
                "motion": {("x", 0, "T+1"), ("y", 0, "T+1")},
                "cambi": {("x", 0, "T"), ("x", 0, "2T+1"), ("x", 1, "T+1"), ("y", 1, "T"), ("y", 2, "T"), ("y", 2, "T+1")}}
OLD_SCENE = {("y", 0, "T-1"), ("y", 0, "T+1")}


def test_vif_at_every_edge():
    def one(w, h, tags, c, k, aligned, _):
        (layout, bits), kind = vif_util.CASES[c], vif_util.CONTENTS[k]
        ref, dis = vif_util.pair(w, h, bits, kind)
        want = vif_ref.vif(ref, dis, bits)
        if aligned:
            got = vif_util.emulate(w, h, layout, bits, wide(vif_util, layout, ref, bits, 11), wide(vif_util, layout, dis, bits, 12))
        else:
            got = test_vif_cpu.emul(w, h, layout, bits, ref, dis, pad=5, dirty=11)
        test_vif_cpu.check_against_restatement(got, want, f"{layout} {bits} {w}x{h} {kind} {'aligned' if aligned else 'odd pitch'}")
    sweep("vif", G.assign(G.vif(), len(vif_util.CASES), len(vif_util.CONTENTS)), one)


def test_adm_at_every_edge():
    def one(w, h, tags, c, k, aligned, _):
        (layout, bits), kind = adm_util.CASES[c], adm_util.CONTENTS[k]
        ref, dis = adm_util.pair(w, h, bits, kind)
        want = adm_ref.adm(ref, dis, bits)
        if aligned:
            got = adm_util.emulate(w, h, layout, bits, wide(adm_util, layout, ref, bits, 11), wide(adm_util, layout, dis, bits, 12))
        else:
            got = test_adm_cpu.emul(w, h, layout, bits, ref, dis, pad=5, dirty=11)
        test_adm_cpu.check_against_restatement(got, want, f"{layout} {bits} {w}x{h} {kind} {'aligned' if aligned else 'odd pitch'}")
    sweep("adm", G.assign(G.adm(), len(adm_util.CASES), len(adm_util.CONTENTS)), one)


def test_motion_at_every_edge():
    """every layout at every size; without padding and clean, with an odd pitch and dirty, and 16-byte aligned and dirty"""
    answers = {}

    def one(w, h, i):
        for c, (layout, bits) in enumerate(motion_util.CASES):
            kind = MOTION_KINDS[(i + c) % len(MOTION_KINDS)]
            if (bits, kind) not in answers:
                seq = motion_util.sequence(w, h, 4, bits, kind)
                answers[bits, kind] = seq, [f[0] for f in motion_ref.sequence(seq, bits)], motion_ref.blur(seq[-1], bits)
            seq, want, blur = answers[bits, kind]
            runs = [test_motion_cpu.emul_seq(w, h, layout, bits, seq, [1, 3], pad=pad, dirty=dirty, want_blur=True) for pad, dirty in ((0, False), (5, True))]
            runs.append(motion_util.emulate(w, h, layout, bits, [1, 3], [wide(motion_util, layout, Y, bits, n) for n, Y in enumerate(seq)], want_blur=True))
            for form, (sads, blurred) in zip(("plain", "odd pitch", "aligned"), runs):
                assert sads == want, (layout, bits, w, h, kind, form)
                assert (blurred == blur).all(), (layout, bits, w, h, kind, form)
        answers.clear()
    sweep("motion", [(w, h, i) for i, (w, h) in enumerate(G.motion())], one)


def test_scene_at_every_edge():
    """every layout at every size, in two of tests/test_scene_cpu.py's four memory forms each; which two alternates with the size and
    with the layout, so every layout meets all four at every edge (an edge has at least two sizes)"""
    variants = lambda layout: ({"pad": 5 if layout != "y10_packed" else 1}, {"aligned": True}, {"vec": False, "pad": 3}, {"pad": 0})

    def one(w, h, i):
        for c, (layout, bits) in enumerate(scene_util.CASES):
            pics = [scene_util.picture(w, h, bits, k, seed=w + h) for k in scene_util.KINDS]  # the four contents as the four slots
            for kw in variants(layout)[(i + c) % 2 * 2:][:2]:
                assert test_scene_cpu.same(test_scene_cpu.emul_hists(w, h, layout, bits, pics, **kw), pics, bits), (w, h, layout, bits, kw)
    sweep("scene", [(w, h, i) for i, (w, h) in enumerate(G.scene())], one)


def test_cambi_at_every_edge():
    def one(w, h, tags, c, k, aligned, b2):
        (layout, bits), kind, window = cambi_util.CASES[c], cambi_util.KINDS[k], G.cambi_window(tags, b2)
        Y = cambi_util.picture(w, h, bits, kind, seed=w + window)
        want = cambi_ref.compute(Y, bits, window, fast=True)  # the whole-plane form, held to the literal one in tests/test_cambi_cpu.py
        if aligned:
            got = cambi_util.emulate(w, h, layout, bits, [1], [wide(cambi_util, layout, Y, bits, 6)], window=window, vec=True)[0]
        else:
            got = test_cambi_cpu._emul1(Y, layout, bits, window, pad=5, dirty=3)
        assert cambi_util.same(got, want), (w, h, layout, bits, kind, window, aligned)
    sweep("cambi", G.assign(G.cambi(), len(cambi_util.CASES), len(cambi_util.KINDS)), one)


def test_xpsnr_at_every_edge():
    """every layout at the sizes below 2^16 samples (the last-block edges); the five large ones (the band edges) rotate them"""
    def one(w, h, tags, c, k, b, _):
        fps, batches = (((25, 1), [2]), ((60, 1), [1, 1]))[b]  # first and second order of the temporal activity
        for c in (range(len(G.XPSNR_CASES)) if w * h < 1 << 16 else [c]):
            layout, bits = G.XPSNR_CASES[c]
            test_xpsnr_cpu._emulated_against_restatement(w, h, layout, bits, fps, batches, pad=(0, 3, 1)[(c + b) % 3], kind=xpsnr_util.KINDS[k], dirty=True)
    sweep("xpsnr", G.assign(G.xpsnr(), len(G.XPSNR_CASES), len(xpsnr_util.KINDS)), one)
