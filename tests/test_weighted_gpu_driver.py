"""tests/weighted_gpu.py, the driver of the weighted chain's GPU tests, still catches what it is for: on an engine whose device memory
is host memory and whose "kernels" are Python, without a GPU."""
import ctypes as C

import numpy as np
import pytest

import weighted_gpu as G


class FakeLib:
    def __init__(self):
        self.error, self.kernel, self.pending = b"", b"", 0

    def gpsx_last_error(self, h):
        return self.error

    def gpsx_last_kernel(self, h):
        return self.kernel

    def gpsx_synchronize(self, h):
        rc, self.pending = self.pending, 0
        return rc


class FakeEngine:
    """capi.Engine's memory calls over numpy arrays: a device address is the array's own"""

    def __init__(self):
        self.lib, self.h, self.live = FakeLib(), None, {}

    def malloc(self, nbytes):
        a = np.zeros(max(nbytes, 1), np.uint8)
        self.live[a.ctypes.data] = a
        return a.ctypes.data

    def free(self, p):
        del self.live[p]

    def h2d(self, p, arr):
        arr = np.ascontiguousarray(arr)
        C.memmove(p, arr.ctypes.data, arr.nbytes)

    def d2h(self, arr, p):
        C.memmove(arr.ctypes.data, p, arr.nbytes)

    def synchronize(self):
        assert self.lib.gpsx_synchronize(self.h) == 0


def poke(address, value=0x11):
    C.memmove(address, bytes([value]), 1)


@pytest.fixture
def fake():
    e = FakeEngine()
    yield e
    assert not e.live, "device memory left allocated"


@pytest.mark.parametrize("device", [True, False])
def test_guarded_sees_one_byte_in_either_canary_and_in_the_payload(fake, device):
    content = np.arange(10, dtype=np.int32)
    for offset in (-1, -G.GUARD, content.nbytes, content.nbytes + G.GUARD - 1):
        with G.Guarded(fake if device else None, content.nbytes, G.STATE_FILL, content) as g:
            assert g.untouched() and g.get(np.int32, 10).tolist() == content.tolist()
            poke(g.ptr.value + offset)
            assert not g.untouched()
            with pytest.raises(AssertionError, match="canary"):
                g.get(np.int32, 10)
    with G.Guarded(fake if device else None, 40) as g:
        assert (g.get(np.uint8, 40) == G.OUT_FILL).all()
        poke(g.ptr.value + 39)
        assert not g.untouched() and g.get(np.uint8, 40)[39] == 0x11      # (a payload byte: seen by untouched(), the canaries stand)
        g.refill()
        assert g.untouched()
        g.put(np.array([7], np.uint8))
        assert g.get(np.uint8, (2,)).tolist() == [7, G.OUT_FILL]


def _stage(fake, dev, past=None, code=0, kernel=b"k_fake"):
    """a stage whose kernel adds the launch's input to the states and writes states + 1 -> run_stage's result.  past: the offset
    behind the output's end of a stray byte"""
    st = np.array([10, 20, 30], np.int32)

    def call(ins, sts, out, k):
        inp = np.frombuffer((C.c_ubyte * 12).from_address(ins[0] if isinstance(ins[0], int) else ins[0].value), np.int32)
        s = np.frombuffer((C.c_ubyte * 12).from_address(sts[0].value), np.int32)
        s += inp
        C.memmove(out.value, (s + 1).tobytes(), 12)
        if past is not None:
            poke(out.value + 12 + past)
        fake.lib.kernel = b"k_fake"
        if dev:
            fake.lib.pending = code
            return 0
        return code
    launches = [([np.array([1, 2, 3], np.int32)], np.int32, (3,)), ([np.array([100, 100, 100], np.int32)], np.int32, (3,))]
    return G.run_stage(fake, call, kernel, st, launches, dev, host_inputs=True)


@pytest.mark.parametrize("dev", [True, False])
def test_run_stage_returns_outputs_states_and_codes_and_sees_a_byte_past_the_output(fake, dev):
    outs, after, codes = _stage(fake, dev)
    assert [o.tolist() for o in outs] == [[12, 23, 34], [112, 123, 134]] and after.tolist() == [111, 122, 133] and codes == [0, 0]
    assert _stage(fake, dev, code=G.EINVAL)[2] == [G.EINVAL, G.EINVAL]      # (the codes as they came: the test judges them)
    for past in (0, G.GUARD - 1):
        with pytest.raises(AssertionError, match="canary"):
            _stage(fake, dev, past=past)
    with pytest.raises(AssertionError):
        _stage(fake, dev, kernel=b"k_other")


def test_run_stage_takes_several_state_arrays_and_a_null(fake):
    a, b = np.array([1, 2], np.int64), np.array([5], np.int16)

    def call(ins, sts, out, k):
        assert sts[1] is None and ins == ["as it is"]
        np.frombuffer((C.c_ubyte * 16).from_address(sts[0].value), np.int64)[:] += 1
        np.frombuffer((C.c_ubyte * 2).from_address(sts[2].value), np.int16)[:] = -7
        fake.lib.kernel = b"k"
        return 0
    outs, afters, codes = G.run_stage(fake, call, b"k", [a, None, b], [(["as it is"], np.uint8, (4,))] * 2, after_each=True)
    assert [s[0].tolist() for s in afters] == [[2, 3], [3, 4]] and afters[1][1] is None and afters[1][2].tolist() == [-7]
    assert all((o == G.OUT_FILL).all() for o in outs) and codes == [0, 0] and a.tolist() == [1, 2]


def _refuse(fake, rc=G.EINVAL, text=None, write=None):
    """refusals() on a call that answers `rc` with `text` (None: the row's) and writes one byte at bufs[write]"""
    by_message = {b"n must be positive": [dict(n=0), dict(n=-1)], b"null argument": [dict(null=True)]}
    calls = []
    with G.Pool() as pool:
        bufs = [pool.add(G.Guarded(fake, 8, G.STATE_FILL, np.arange(8, dtype=np.uint8))), pool.add(G.Guarded(fake, 16)), pool.add(G.Guarded(None, 16))]

        def call(a, dev):
            calls.append((dev, a["n"], a["null"]))
            fake.lib.error = text or (b"null argument" if a["null"] else b"n must be positive")
            if write is not None:
                poke(bufs[write].ptr.value + 3)
            return rc
        G.refusals(fake, by_message, dict(n=4, null=False), call, bufs)
    return calls


def test_refusals_runs_every_row_in_both_variants_and_fails_on_a_byte_a_text_or_a_code(fake):
    assert _refuse(fake) == [(dev, n, null) for dev in (False, True) for n, null in ((0, False), (-1, False), (4, True))]
    for write in (0, 1, 2):      # (a state, a device output, a host output)
        with pytest.raises(AssertionError):
            _refuse(fake, write=write)
    with pytest.raises(AssertionError):
        _refuse(fake, text=b"n must be positive ")
    for rc in (0, -1):
        with pytest.raises(AssertionError):
            _refuse(fake, rc=rc)


def test_same_rows_and_columns_name_the_first_difference():
    want = np.zeros((3, 5), np.int32)
    got = want.copy()
    G.same_columns(got, want, "equal")
    G.same_rows(got[0], want[0], "equal")
    got[2, 3] = got[1, 4] = 1
    with pytest.raises(AssertionError) as e:
        G.same_columns(got, want, "records")
    assert e.value.args[0][:2] == ("records", [3, 4]) and e.value.args[0][3] == 2
    G.same_columns(got, want, "the others", channels=[0, 1, 2])
    with pytest.raises(AssertionError) as e:
        G.same_rows(got[2], want[2], "states", names=list("abcde"))
    assert e.value.args[0][:3] == ("states", [3], "d")
