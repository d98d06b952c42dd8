"""GPU tier of the edge-geometry sweep: every feature library on the MI355X against its numpy restatement at the sizes of
tests/geom_sweep.py (the picture edge one short of, on and just past a tile boundary, at every scale), one engine per size at batch 2,
the planes handed over as device memory, alternately with an aligned base and pitch and with a base one element off and an odd pitch.
What alternates is geom_sweep.assign's bit, the parity of an entry's rank among the entries of its own edge, NOT the parity of the list
index (with eight layouts that is the layout's own parity): tests/test_geom_sweep_cpu.py::test_the_rotation_reaches_every_load_path holds
that every layout meets both forms, and every storage format both forms at every x edge (the thinned CAMBI list: at every x edge but
y8 unaligned at exactly T).  Motion and scene run EVERY layout at every size, the form alternating with size and layout; XPSNR runs every
layout at the sizes below 2^16 samples (the last-block edges) and rotates them over the five large ones (the band edges).  Each comparison is the library's own GPU test's: motion, scene and XPSNR bit-identical, VIF within RTOL, ADM within
rtol(area), CAMBI's heat maps equal and cambi within 1e-9.

The restatements are the cost.  Measured on one CPU core for the full lists, one picture or sequence per size
(tests/test_geom_sweep_cpu.py prints it); a test here computes two per size, one per slot:
    vif 171 sizes 4.7 s     adm 181 sizes 1.9 s     cambi 215 sizes 26 s     motion 33 sizes 0.1 s     scene 36 sizes < 0.1 s
    xpsnr 21 sizes 3 s, nearly all of it the five 0.6-megapixel pictures whose blocks a band of rows splits
Twice that is within about ten seconds for every library but CAMBI, so only CAMBI's list is thinned, by the rule of
tests/geom_sweep.py (`drop=`: a size goes only if EVERY edge it stands for may go, and only a 2T-1 / 2T+1 entry or an odd variant may;
no T-1 / T / T+1 / T+r entry and no per-library extra is dropped):
    cambi      the 2T-1 / 2T+1 entries of scales >= 2, then every odd variant: 130 of 215 sizes stay, about 15 s per slot
    vif, adm, motion, scene, xpsnr   nothing
What is left of CAMBI's is still more than ten seconds of restatement on that core: nothing else may go by the rule, so it stays.  (The
hosts of the MI355X have faster cores: the whole CAMBI test, both slots, took 4.7 s there.)
The CPU tier runs the full lists."""
import time

import pytest

from tests import adm_ref, adm_util, cambi_ref, cambi_util, geom_sweep as G, motion_ref, motion_util, scene_util, vif_ref, vif_util
from tests import test_gpu_adm, test_gpu_cambi, test_gpu_motion, test_gpu_scene, test_gpu_vif, test_gpu_xpsnr
from tests import xpsnr_ref, xpsnr_util
from tests.test_geom_sweep_cpu import MOTION_KINDS
from tests.test_gpu_motion import _hand_over
from tm_pkg import tm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _done(name, sizes, ran, t0, t_ref):
    print(f"{name}: {ran} sizes, {time.time() - t0:.1f} s, of which the restatement {t_ref:.1f} s")
    assert ran == len(sizes) and ran > 0


def _pair_sweep(name, sizes, U, cls, ref_fn, close, set_pair):
    t0, t_ref, ran = time.time(), 0.0, 0
    for w, h, _, c, k, unaligned, _ in G.assign(sizes, len(U.CASES), len(U.CONTENTS)):
        (layout, bits), kind = U.CASES[c], U.CONTENTS[k]
        pairs = [U.pair(w, h, bits, U.CONTENTS[0], seed=7), U.pair(w, h, bits, kind)]  # slot 0: noise; slot 1: this entry's kind
        with cls(w, h, layout, bits, batch=2) as v:
            keep = [set_pair(v, s, layout, bits, *pairs[s], mem="device", aligned=not unaligned, pad=3, dirty=5 + 2 * s) for s in range(2)]
            v.compute(2)
            frames = v.frames(2)
            del keep
        for s in range(2):
            t = time.time()
            want = ref_fn(*pairs[s], bits)
            t_ref += time.time() - t
            close(frames[s], want, w, h, f"{layout} {bits} {w}x{h} slot {s} {kind if s else 'noise'} {'unaligned' if unaligned else 'aligned'}")
        ran += 1
    _done(name, sizes, ran, t0, t_ref)


def test_vif_at_every_edge():
    assert vif_util.CONTENTS[0] == "noise"
    _pair_sweep("vif", G.vif(), vif_util, tm.Vif, vif_ref.vif, lambda g, x, w, h, what: test_gpu_vif._close(g, x, what),
                test_gpu_vif._set)


def test_adm_at_every_edge():
    assert adm_util.CONTENTS[0] == "noise"
    _pair_sweep("adm", G.adm(), adm_util, tm.Adm, adm_ref.adm, test_gpu_adm._close, test_gpu_adm._set)


def test_motion_at_every_edge():
    sizes, t0, t_ref, ran = G.motion(), time.time(), 0.0, 0
    for i, (w, h) in enumerate(sizes):
        answers = {}
        for c, (layout, bits) in enumerate(motion_util.CASES):
            kind = MOTION_KINDS[(i + c) % len(MOTION_KINDS)]
            if (bits, kind) not in answers:
                t = time.time()
                seq = motion_util.sequence(w, h, 2, bits, kind)
                answers[bits, kind] = seq, motion_ref.sequence(seq, bits)
                t_ref += time.time() - t
            seq, want = answers[bits, kind]
            with tm.Motion(w, h, layout, bits, batch=2) as m:
                assert test_gpu_motion._run(m, layout, bits, seq, [2], "device", (i + c) % 2 == 0, pad=3) == want, (w, h, layout, bits, kind)
        ran += 1
    _done("motion", sizes, ran, t0, t_ref)


def test_scene_at_every_edge():
    sizes, t0, ran = G.scene(), time.time(), 0
    for i, (w, h) in enumerate(sizes):
        for c, (layout, bits) in enumerate(scene_util.CASES):
            kind = scene_util.KINDS[(i + c) % len(scene_util.KINDS)]
            pics = [scene_util.picture(w, h, bits, "noise", seed=w + h), scene_util.picture(w, h, bits, kind, seed=w + h + 1)]
            with tm.Scene(w, h, layout, bits, batch=2) as s:
                got = test_gpu_scene._compute(s, layout, bits, pics, "device", (i + c) % 2 == 0, pad=3 if layout != "y10_packed" else 0)
                assert test_gpu_scene._same(got, pics, bits), (w, h, layout, bits, kind)
        ran += 1
    _done("scene", sizes, ran, t0, 0.0)


def test_cambi_at_every_edge():
    sizes, t0, t_ref, ran = G.cambi(drop=G.deep_doubles_and_odd), time.time(), 0.0, 0
    for w, h, tags, c, k, unaligned, b2 in G.assign(sizes, len(cambi_util.CASES), len(cambi_util.KINDS)):
        (layout, bits), kind, window = cambi_util.CASES[c], cambi_util.KINDS[k], G.cambi_window(tags, b2)
        pics = [cambi_util.picture(w, h, bits, "noise", seed=w + window), cambi_util.picture(w, h, bits, kind, seed=w + window)]
        with tm.Cambi(w, h, layout, bits, window=window, batch=2) as cam:
            assert cam.window == window
            got = test_gpu_cambi._compute(cam, layout, bits, pics, "device", not unaligned, pad=3 if layout != "y10_packed" else 0)
        for g, Y in zip(got, pics):
            t = time.time()
            want = cambi_ref.compute(Y, bits, window, fast=True)
            t_ref += time.time() - t
            assert test_gpu_cambi._same(g, want), (w, h, layout, bits, kind, window, unaligned)
        ran += 1
    _done("cambi", sizes, ran, t0, t_ref)


def test_xpsnr_at_every_edge():
    sizes, t0, t_ref, ran = G.xpsnr(), time.time(), 0.0, 0
    for i, (w, h, _, c, k, b, _) in enumerate(G.assign(sizes, len(G.XPSNR_CASES), len(xpsnr_util.KINDS))):
        kind, fps, answers = xpsnr_util.KINDS[k], ((25, 1), (60, 1))[b], {}
        for c in (range(len(G.XPSNR_CASES)) if w * h < 1 << 16 else [c]):
            layout, bits = G.XPSNR_CASES[c]
            if bits not in answers:
                t = time.time()
                pics = [xpsnr_util.pictures(w, h, 0, bits, "random"), xpsnr_util.pictures(w, h, 1, bits, kind)]
                seq = xpsnr_ref.Sequence(w, h, bits, fps)
                answers[bits] = pics, [seq.push(r, d) for r, d in pics]
                t_ref += time.time() - t
            pics, want = answers[bits]
            with tm.Xpsnr(w, h, layout, bits, fps=fps, batch=2) as x:
                keep = []
                for s, pair in enumerate(pics):
                    planes = [[_hand_over(p, "device", (i + c) % 2 == 0) for p in xpsnr_util.layout_planes(layout, side, w, h, bits, 3, dirty=xpsnr_util.dirt_seed(s, n))]
                              for n, side in enumerate(pair)]
                    x.set_pair(s, *planes)
                    keep.append(planes)
                x.compute(2)
                test_gpu_xpsnr._check(x.frames(2), want)
                del keep
        ran += 1
    _done("xpsnr", sizes, ran, t0, t_ref)
