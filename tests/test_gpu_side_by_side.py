"""The six feature libraries (XPSNR, motion, VIF, ADM, scene, CAMBI) in flight together on the MI355X, as the CLI drives them: the same
device surfaces under several objects, every compute_async before any sync, one host thread per library, two objects of one library
with different geometry interleaved, and a result read without an explicit sync.  Every comparison is bit identity with the same
object's answer when it runs alone (compute, sync, read, nothing else in flight): the libraries use no floating-point atomics and a
fixed summation order, so no tolerance is needed or allowed.  One process, at most six host threads, pictures of 96 x 64 and 131 x 70."""
import threading

import numpy as np
import pytest

from tests import cambi_util, xpsnr_util
from tests.test_gpu_motion import _hand_over
from tm_pkg import tm

pytestmark = pytest.mark.gpu

BATCH = 3
NAMES = ("xpsnr", "motion", "vif", "adm", "scene", "cambi")
SIZES = [(96, 64), (131, 70)]


@pytest.fixture(scope="module", autouse=True)
def _hip():
    tm.init_hip(0)


def _bits(x):
    """a result as something == compares bit for bit: doubles by their hex text (a NaN equals itself, -0.0 is not 0.0), arrays by
    their bytes"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    return x


class Inputs:
    """`n` reference / distorted pictures of w x h as device tensors: the luma planes (layout y8 at 8 bits, y16_msb above) that every
    library reads, and the interleaved chroma that only XPSNR (nv12 / p016: the same luma plane) reads.  The distorted lumas are
    CAMBI's contents (steps, steps and noise, noise) so that no library's answer is trivial; a reference is its distorted picture plus
    a little noise."""

    def __init__(self, w, h, bits, seed, n=BATCH):
        self.w, self.h, self.bits = w, h, bits
        self.layout, self.xlayout = ("y8", "nv12") if bits == 8 else ("y16_msb", "p016")
        rng = np.random.default_rng([0x51DE, seed, w, h, bits])
        M = (1 << bits) - 1
        cw, ch = (w + 1) // 2, (h + 1) // 2
        self.pairs = []
        for i in range(n):
            dis = cambi_util.picture(w, h, bits, ("mixed", "stairs_lo", "noise")[i % 3], seed=seed + i)
            ref = np.clip(dis + rng.integers(-(M // 64) - 1, M // 64 + 2, (h, w)), 0, M)
            sides = []
            for Y in (ref, dis):
                planes = xpsnr_util.layout_planes(self.xlayout, (Y, rng.integers(0, M + 1, (ch, cw)), rng.integers(0, M + 1, (ch, cw))), w, h, bits)
                sides.append(tuple(_hand_over(p, "device", True) for p in planes))  # (luma, CbCr)
            self.pairs.append(tuple(sides))


def make(name, inp):
    a = (inp.w, inp.h, inp.layout, inp.bits)
    if name == "xpsnr":
        return tm.Xpsnr(inp.w, inp.h, inp.xlayout, inp.bits, fps=(60, 1), batch=BATCH)
    if name == "cambi":
        return tm.Cambi(*a, window=7, batch=BATCH)
    return {"motion": tm.Motion, "vif": tm.Vif, "adm": tm.Adm, "scene": tm.Scene}[name](*a, batch=BATCH)


def set_slots(name, e, inp, order):
    """slot s takes pair order[s]; motion, scene and CAMBI take the distorted luma"""
    for s, i in enumerate(order):
        (ry, rc), (dy, dc) = inp.pairs[i]
        if name == "xpsnr":
            e.set_pair(s, (ry, rc), (dy, dc))
        elif name in ("vif", "adm"):
            e.set_pair(s, ry, dy)
        else:
            e.set_frame(s, dy)


def read(name, e, n=BATCH):
    out = [_bits(tuple(f)) for f in e.frames(n)]
    if name == "cambi":
        out += [_bits(e.heatmap(i, s)) for i in range(n) for s in range(5)]
    return out


def order_of(r):
    """the pairs of compute r: a rotation, so that the sequences of motion and XPSNR (which keep history) differ from round to round"""
    return [(s + r) % BATCH for s in range(BATCH)]


def solo(name, inp, rounds):
    """the answers of `rounds` computes of one object with nothing else in flight"""
    out = []
    with make(name, inp) as e:
        for r in range(rounds):
            set_slots(name, e, inp, order_of(r))
            e.compute(BATCH)
            out.append(read(name, e))
    return out


@pytest.fixture(scope="module")
def alone():
    """inputs and solo answers (20 computes each), computed once per size and shared by the tests below"""
    cache = {}

    def get(w, h, bits=10, seed=0):
        key = (w, h, bits, seed)
        if key not in cache:
            inp = Inputs(w, h, bits, seed)
            cache[key] = (inp, {name: solo(name, inp, 20) for name in NAMES})
        return cache[key]
    return get


def test_the_solo_answers_tell_slots_and_rounds_apart(alone):
    for w, h in SIZES:
        _, want = alone(w, h)
        for name in NAMES:
            frames = want[name][0][:BATCH]
            assert len(set(frames)) == BATCH, name                                   # three slots, three answers
            assert want[name][0] != want[name][1], name                              # another order of the pairs, another answer
        for name in ("motion", "xpsnr"):                                             # history: the same pairs after other pictures
            assert want[name][0] != want[name][3] and want[name][3] == want[name][6], name
        for name in ("vif", "adm", "scene", "cambi"):
            assert want[name][0] == want[name][3], name


@pytest.mark.parametrize("w,h", SIZES)
def test_all_six_on_the_same_surfaces(alone, w, h):
    inp, want = alone(w, h)
    engines = {name: make(name, inp) for name in NAMES}
    try:
        for r in range(3):
            for name, e in engines.items():
                set_slots(name, e, inp, order_of(r))
            for e in engines.values():
                e.compute_async(BATCH)
            for e in engines.values():
                e.sync()
            for name, e in engines.items():
                assert read(name, e) == want[name][r], (name, r)
    finally:
        for e in engines.values():
            e.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_one_thread_per_library(alone, w, h):
    inp, want = alone(w, h)
    engines = {name: make(name, inp) for name in NAMES}
    errors = []

    def worker(name):
        try:
            e = engines[name]
            if hasattr(e, "reset"):
                e.reset()
            for r in range(20):
                set_slots(name, e, inp, order_of(r))
                e.compute_async(BATCH)
                e.sync()
                if read(name, e) != want[name][r]:
                    raise AssertionError(f"{name} compute {r}")
        except Exception as exc:  # noqa: BLE001 -- reported below, in the main thread
            errors.append(exc)
    th = [threading.Thread(target=worker, args=(name,)) for name in NAMES]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for e in engines.values():
        e.close()
    assert not errors, errors


@pytest.mark.parametrize("name", NAMES)
def test_two_engines_of_one_library_with_different_geometry(alone, name):
    (ia, wa), (ib, wb) = alone(96, 64, 8), alone(131, 70, 10)
    with make(name, ia) as a, make(name, ib) as b:
        for r, first in enumerate((a, b)):
            second = b if first is a else a
            set_slots(name, a, ia, order_of(r))
            set_slots(name, b, ib, order_of(r))
            first.compute_async(BATCH)
            second.compute_async(BATCH)
            second.sync()
            first.sync()
            assert read(name, a) == wa[name][r], (name, "A", r)
            assert read(name, b) == wb[name][r], (name, "B", r)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("name", ["vif", "adm", "cambi"])
def test_a_result_belongs_to_its_compute(alone, name, w, h):
    """no explicit sync: the getters wait for the object's own stream; other pairs set right behind them do not reach back"""
    (ip, wp), (iq, wq) = alone(w, h), alone(w, h, seed=50)
    assert wp[name][0] != wq[name][0]
    with make(name, ip) as e:
        for inp, want in ((ip, wp), (iq, wq)):
            set_slots(name, e, inp, order_of(0))
            e.compute_async(BATCH)
            got = [_bits(tuple(f)) for f in e.frames(BATCH)]
            assert got == want[name][0][:BATCH], name
