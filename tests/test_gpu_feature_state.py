"""The state machine the ten feature libraries share (set, compute_async, sync, get), through each binding on the MI355X at 96 x 64,
8 bits, batch 2, with host pictures (so the staging surfaces are in play).  What is expected here is what the libraries did before
they shared one host core (csrc/tm_feature_host.h): the test was written against that commit and passed there.

All ten hand every slot over anew before each compute.  XPSNR's struct once commented its `have` flags as "set since create"; its
compute cleared them like everybody else's and include/turbo_metrics_xpsnr.h documents TM_ERR_STATE, so it is held to the same rule.

No call here makes a HIP call fail: every refusal is decided on the host before anything is queued."""
import pytest

from tests import adm_util, cambi_util, ciede_util, flip_util, hvs_util, motion_util, scene_util, vif_util, xpsnr_util, yuv_util
from tests.test_gpu_side_by_side import _bits
from tm_pkg import tm

pytestmark = pytest.mark.gpu

W, H, BITS, BATCH = 96, 64, 8, 2
NAMES = ("xpsnr", "motion", "vif", "adm", "scene", "cambi", "flip", "yuv", "hvs", "ciede")


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _luma(Y):
    return motion_util.luma_plane("y8", Y, BITS)


def make(name):
    """(the object, [what slot i is set with]): host numpy planes"""
    a = (W, H, "y8", BITS)
    if name == "xpsnr":
        pics = [xpsnr_util.pictures(W, H, i, BITS) for i in range(BATCH)]
        return tm.Xpsnr(W, H, "nv12", BITS, fps=(60, 1), batch=BATCH), [tuple(xpsnr_util.layout_planes("nv12", p, W, H, BITS) for p in pr) for pr in pics]
    if name == "motion":
        return tm.Motion(*a, batch=BATCH), [(_luma(Y),) for Y in motion_util.sequence(W, H, BATCH, BITS)]
    if name in ("vif", "adm", "hvs"):
        cls, pair, kind = {"vif": (tm.Vif, vif_util.pair, "blurred"), "adm": (tm.Adm, adm_util.pair, "blurred"), "hvs": (tm.Hvs, hvs_util.pair, "noise")}[name]
        return cls(*a, batch=BATCH), [tuple(_luma(Y) for Y in pair(W, H, BITS, kind, seed=i)) for i in range(BATCH)]
    if name == "scene":
        return tm.Scene(*a, batch=BATCH), [(_luma(scene_util.picture(W, H, BITS, "smooth", seed=i)),) for i in range(BATCH)]
    if name == "cambi":
        return tm.Cambi(*a, window=7, batch=BATCH), [(_luma(cambi_util.picture(W, H, BITS, "mixed", seed=i)),) for i in range(BATCH)]
    if name == "flip":
        return tm.Flip(W, H, batch=BATCH), [flip_util.pair(W, H, "smooth", seed=i) for i in range(BATCH)]
    U, cls = {"yuv": (yuv_util, tm.Yuv), "ciede": (ciede_util, tm.Ciede)}[name]
    return cls(W, H, "nv12", BITS, batch=BATCH), U.frames_of("nv12", [U.pair(W, H, BITS, "noise", seed=i) for i in range(BATCH)], W, H, BITS)


def feed(e, slot, what):
    (e.set_pair if len(what) == 2 else e.set_frame)(slot, *what)


def refused(call):
    """the call raises the binding's error with TM_ERR_STATE"""
    with pytest.raises(RuntimeError) as err:
        call()
    assert err.value.code == tm.ffi.TM_ERR_STATE, err.value
    return True


@pytest.mark.parametrize("name", NAMES)
def test_state_machine(name):
    e, inputs = make(name)
    with e:
        feed(e, 0, inputs[0])
        assert refused(lambda: e.compute_async(BATCH))      # slot 1 was never set
        assert refused(lambda: e.frames(1))                 # nothing was computed yet
        feed(e, 1, inputs[1])
        e.compute_async(BATCH)
        assert refused(lambda: e.compute_async(BATCH))      # one compute at a time
        e.sync()
        first = [_bits(tuple(f)) for f in e.frames(BATCH)]
        mem = e.mem_usage()
        assert mem > 0
        assert refused(lambda: e.frames(BATCH + 1))         # beyond the last compute
        assert refused(lambda: e.frames(1, first=BATCH))
        assert [_bits(tuple(f)) for f in e.frames(1, first=1)] == first[1:]

        assert refused(lambda: e.compute_async(BATCH))      # the compute consumed its slots
        assert refused(lambda: e.compute_async(1))
        feed(e, 1, inputs[1])
        assert refused(lambda: e.compute_async(BATCH))      # slot 0 was not set again
        if hasattr(e, "reset"):                             # the sequences (motion, XPSNR) start over; reset forgets the slots
            e.reset()
            feed(e, 0, inputs[0])
            assert refused(lambda: e.compute_async(BATCH))
            feed(e, 1, inputs[1])
        feed(e, 0, inputs[0])
        e.compute_async(BATCH)
        e.sync()
        assert [_bits(tuple(f)) for f in e.frames(BATCH)] == first
        assert e.mem_usage() == mem

        feed(e, 0, inputs[0])
        e.compute_async(1)                                  # a shorter compute moves the limit
        assert refused(lambda: e.frames(BATCH))
        assert len(e.frames(1)) == 1                        # waits for the compute by itself
        assert e.mem_usage() == mem
