"""What the GPU tests of the weighted chain's stages share (tests/test_gpu_weighted_{loop,sync,aided,forced,multi,nav,obs,eph,lock,fix,
pvt}.py): the engine fixture, memory between canaries, the launch-after-launch driver of one stage in its _dev and its host
variant, the loop over a stage's refusals, the per-channel comparison, and the device chain from IF samples onwards.  A test file
keeps its cases, its order of calls and its assertions.  tests/test_weighted_gpu_driver.py holds this module to what it is for, on a
fake engine and without a GPU."""
import ctypes as C

import numpy as np
import pytest

import weighted_eph_ref as E
import weighted_lock_ref as R
import weighted_nav_ref as N
import weighted_obs_ref as O
import weighted_sync_ref as Y

GUARD = 4096      # bytes of canary on either side
EINVAL = -22
STATE_FILL, OUT_FILL = 0x5A, 0xA5      # the canaries around states and inputs; the canaries around outputs and their prefill


@pytest.fixture(scope="module")
def eng():
    """one engine per test module (a module imports this name; the scope is the importing module's)"""
    from stm32f4_sdr_gps_amd import capi
    e = capi.Engine(0)
    yield e
    e.close()


class Guarded:
    """`nbytes` of device memory -- of host memory when `eng` is None -- between two canaries of GUARD bytes; the payload starts as
    `content` or as the fill byte.  `image` is that start: canaries, and content or prefill"""

    def __init__(self, eng, nbytes, fill=OUT_FILL, content=None):
        self.eng, self.nbytes, self.fill = eng, nbytes, fill
        self.image = np.full(GUARD + nbytes + GUARD, fill, np.uint8)
        if content is not None:
            self.image[GUARD:GUARD + nbytes] = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        self.mem = np.empty_like(self.image) if eng is None else None
        self.base = self.mem.ctypes.data if eng is None else eng.malloc(self.image.nbytes)
        self.ptr = C.c_void_p(self.base + GUARD)
        self.refill()

    def refill(self):
        """the canaries and the payload as they were at the start"""
        if self.eng is None:
            self.mem[:] = self.image
        else:
            self.eng.h2d(self.base, self.image)

    def put(self, content):
        """`content` from the payload's first byte on"""
        if self.eng is None:
            self.mem[GUARD:GUARD + content.nbytes] = np.ascontiguousarray(content).view(np.uint8).reshape(-1)
        else:
            self.eng.h2d(self.base + GUARD, content)

    def _now(self):
        if self.eng is None:
            return self.mem
        now = np.empty_like(self.image)
        self.eng.d2h(now, self.base)
        return now

    def get(self, dtype, shape):
        """the payload's first prod(shape) items, after a look at both canaries"""
        now = self._now()
        assert (now[:GUARD] == self.fill).all() and (now[GUARD + self.nbytes:] == self.fill).all(), "a canary was written"
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert n <= self.nbytes
        return now[GUARD:GUARD + n].view(dtype).reshape(shape).copy()

    def untouched(self):
        """no byte, canaries included, differs from what the buffer started as"""
        return bool((self._now() == self.image).all())

    def free(self):
        if self.eng is not None:
            self.eng.free(self.base)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class Pool(list):
    """Guarded buffers that are freed together: `with Pool() as pool: a = pool.add(Guarded(...))`"""

    def add(self, buf):
        self.append(buf)
        return buf

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self:
            if buf is not None:
                buf.free()


def run_stage(eng, call, kernel, states, launches, dev=True, host_inputs=False, after_each=False):
    """One stage, launch after launch, on copies of `states` in device memory: one array or a list of them (None: a NULL pointer), as
    the call takes them (lock states and sync states, say).  launches: [(inputs, out dtype, out shape)]; an input is an array --
    uploaded for the launch; with host_inputs (the block-taking stages) the host variant gets its address instead -- or anything
    else, which is passed on as it is (an address inside a buffer the test uploaded).  call(inputs, states, out, k) -> the return
    code of launch k's _dev call (dev) or host call on these pointers.  States and outputs sit between canaries, the outputs are prefilled;
    the host variant's output is host memory.  The _dev call must return 0 and the code kept is gpsx_synchronize's; the host call's
    code is kept as it is; either must have run `kernel`.
    -> ([output per launch], states after -- after every launch with after_each --, [codes]); states in the form they were given"""
    several = isinstance(states, (list, tuple))
    given = list(states) if several else [states]
    with Pool() as sts:
        for s in given:
            sts.append(None if s is None else Guarded(eng, s.nbytes, STATE_FILL, s))

        def read_states():
            now = [None if g is None else g.get(s.dtype, s.shape) for g, s in zip(sts, given)]
            return now if several else now[0]
        outs, afters, codes = [], [], []
        for k, (inputs, dtype, shape) in enumerate(launches):
            uploaded, p_in = [], []
            try:
                for a in inputs:
                    if not isinstance(a, np.ndarray):
                        p_in.append(a)
                    elif host_inputs and not dev:
                        p_in.append(a.ctypes.data)
                    else:
                        uploaded.append(eng.malloc(a.nbytes))
                        eng.h2d(uploaded[-1], a)
                        p_in.append(C.c_void_p(uploaded[-1]))
                with Guarded(eng if dev else None, int(np.prod(shape)) * np.dtype(dtype).itemsize) as out:
                    rc = call(p_in, [None if g is None else g.ptr for g in sts], out.ptr, k)
                    if dev:
                        assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
                    assert eng.lib.gpsx_last_kernel(eng.h) == kernel
                    codes.append(eng.lib.gpsx_synchronize(eng.h) if dev else rc)
                    outs.append(out.get(dtype, shape))
            finally:
                for p in uploaded:
                    eng.free(p)
            if after_each:
                afters.append(read_states())
        return outs, (afters if after_each else read_states()), codes


def block_launches(blocks, pieces, dtype, shape_of):
    """run_stage's launches for a block-taking stage: `blocks` cut into consecutive launches of `pieces` blocks (None: one launch),
    the output of a launch of k blocks being dtype [shape_of(k)] -> (launches, [first block per launch])"""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, 4092)
    launches, firsts, at = [], [], 0
    for k in pieces or [len(blocks)]:
        launches.append(([blocks[at:at + k]], dtype, shape_of(k)))      # (a slice of whole blocks: contiguous)
        firsts.append(at)
        at += k
    return launches, firsts


def refusals(eng, by_message, good, call, bufs):
    """Every refusal with its exact text writes nothing.  by_message: {text: [changes to the `good` arguments]}; call(a, dev) makes
    the host (dev False) or the _dev call from the argument dict a = {**good, **change} -> its return code; bufs: the Guarded
    buffers, device or host, that a call may write: states and outputs.  Per variant and row: the buffers as they were at the
    start, the call, GPSX_EINVAL and gpsx_last_error equal to the row's text, a synchronize, and no byte of any buffer changed"""
    for dev in (False, True):
        for message, changes in by_message.items():
            for change in changes:
                for b in bufs:
                    b.refill()
                rc = call({**good, **change}, dev)
                assert rc == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (dev, change, rc, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()      # nothing was enqueued, nothing is pending
                assert all(b.untouched() for b in bufs), (dev, change, [i for i, b in enumerate(bufs) if not b.untouched()])


def same_rows(got, want, what, channels=None, names=None):
    """one item per channel (states, observables, ephemeris and lock records), byte for byte; names the first channels that differ"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if channels is None and got.tobytes() == np.ascontiguousarray(want).tobytes():
        return
    bad = [c for c in (range(len(got)) if channels is None else channels) if got[c:c + 1].tobytes() != want[c:c + 1].tobytes()]
    assert not bad, (what, bad[:4], names and names[bad[0]], got[bad[0]], want[bad[0]])


def same_columns(got, want, what, channels=None, names=None):
    """records [slot][channel], byte for byte per channel; names the first channels that differ and the first slot of the first"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if channels is None and got.tobytes() == np.ascontiguousarray(want).tobytes():
        return
    bad = [c for c in (range(got.shape[1]) if channels is None else channels) if got[:, c].tobytes() != want[:, c].tobytes()]
    if bad:
        slot = [u for u in range(got.shape[0]) if got[u, bad[0]].tobytes() != want[u, bad[0]].tobytes()][0]
        assert not bad, (what, bad[:4], names and names[bad[0]], slot, got[slot, bad[0]], want[slot, bad[0]])


def sync_cfg(c):
    """a restatement's cfg dict (weighted_sync_ref.make_cfg) -> the library's gpsx_wsync_cfg_t"""
    from stm32f4_sdr_gps_amd import capi
    gains = {name: dict(dll=(c[name]["dll_c1"], c[name]["dll_c2"]), pll=(c[name]["pll_c1"], c[name]["pll_c2"]), fll=c[name]["fll_c"]) for name in ("search", "lock")}
    return capi.wsync_cfg(c["n_coh_search"], c["n_coh_lock"], gains["search"], gains["lock"], c["sync_bits"], (c["sync_num"], c["sync_den"]),
                          c["use_magnitude"], c["spacing"])


class Chain:
    """The device chain behind one IF stream: the sync loop's states and those of the stages asked for (`states`: {"sync": ..,
    "nav": .., "obs": .., "eph": .., "lock": ..}) between canaries, and one guarded, prefilled output buffer per stage, sized for
    launches of up to max_blocks blocks.  A stage's method enqueues its _dev call on these buffers for the launch that sync() -- or
    records(), with sync records made on the CPU -- began; the test decides the order, synchronizes and reads: read(name) -> a
    state array, or "rec" / "words" / "o" / "e" / "l": the last launch's sync records, words, observables, ephemeris and lock records."""
    OUT = dict(rec=Y.REC_DTYPE, words=N.WORD_DTYPE, o=O.OBS_DTYPE, e=E.EPH_DTYPE, l=R.LOCK_DTYPE)

    def __init__(self, eng, sync_cfg, states, max_blocks, max_bad_words=3, edge_guard=512.0, lock_cfg=None, rx=None, max_slots=None):
        """sync_cfg None: no sync stage, a launch has up to max_slots record slots"""
        from stm32f4_sdr_gps_amd import capi
        self.eng, self.sync_cfg, self.lock_cfg, self.rx, self.states = eng, sync_cfg, lock_cfg, rx, states
        self.n_ch, self.n, self.n_slots = len(next(iter(states.values()))), 0, 0
        self.span = None if sync_cfg is None else (int(sync_cfg["n_coh_search"][0]), int(sync_cfg["n_coh_lock"][0]))
        self.nav_cfg, self.obs_cfg, self.eph_cfg = np.zeros(1, capi.WNAV_CFG_DTYPE), np.zeros(1, capi.WOBS_CFG_DTYPE), np.zeros(1, capi.WEPH_CFG_DTYPE)
        self.nav_cfg["max_bad_words"], self.obs_cfg["edge_guard"] = max_bad_words, edge_guard
        self.buf = {}
        try:
            for name, st in states.items():
                self.buf[name] = Guarded(eng, st.nbytes, STATE_FILL, st)
            items = dict(rec=max_slots or capi.wsync_slots(max_blocks, *self.span), words=N.max_words(max_blocks))
            for name, dtype in self.OUT.items():
                self.buf[name] = Guarded(eng, items.get(name, 1) * self.n_ch * dtype.itemsize)
        except BaseException:
            self.free()
            raise

    def shape(self, name):
        return {"rec": (self.n_slots, self.n_ch), "words": (N.max_words(self.n), self.n_ch)}.get(name, (self.n_ch,))

    def begin(self, n):
        """a launch of n blocks: what read() and the stages' calls size by"""
        from stm32f4_sdr_gps_amd import capi
        self.n, self.n_slots = n, capi.wsync_slots(n, *self.span)

    def _enqueue(self, name, *args):
        self.eng._chk(getattr(self.eng.lib, name)(self.eng.h, *args), name)

    def sync(self, d_if_at, n):
        """begins a launch of n blocks at device address d_if_at: the sync loop (with `rx`, for many receivers, unaided)"""
        self.begin(n)
        if self.rx is None:
            self._enqueue("gpsx_track_loop_weighted_sync_dev", self.sync_cfg.ctypes.data, C.c_void_p(d_if_at), n, self.buf["sync"].ptr, self.n_ch,
                          self.buf["rec"].ptr)
        else:
            self._enqueue("gpsx_track_loop_weighted_sync_multi_dev", self.sync_cfg.ctypes.data, None, self.rx.ctypes.data, C.c_void_p(d_if_at), n,
                          self.buf["sync"].ptr, self.buf["rec"].ptr)

    def records(self, rec, n):
        """begins a launch of n blocks with these sync records"""
        self.n, self.n_slots = n, rec.shape[0]
        self.buf["rec"].put(rec)

    def words(self):
        self._enqueue("gpsx_wnav_words_dev", self.nav_cfg.ctypes.data, self.buf["rec"].ptr, self.n_slots, self.n, self.buf["nav"].ptr, self.n_ch,
                      self.buf["words"].ptr)

    def obs(self):
        self._enqueue("gpsx_wobs_dev", self.obs_cfg.ctypes.data, self.buf["rec"].ptr, self.n_slots, self.n, self.buf["words"].ptr,
                      self.buf["obs"].ptr, self.n_ch, self.buf["o"].ptr)

    def eph(self):
        self._enqueue("gpsx_weph_dev", self.eph_cfg.ctypes.data, self.buf["words"].ptr, self.n, self.buf["eph"].ptr, self.n_ch, self.buf["e"].ptr)

    def lock(self, rearm_on_sync=False):
        """rearm_on_sync: the lock stage gets the sync states to re-arm; else a NULL pointer"""
        self._enqueue("gpsx_wlock_dev", self.lock_cfg.ctypes.data, self.buf["rec"].ptr, self.n_slots, self.n, self.buf["lock"].ptr,
                      self.buf["sync"].ptr if rearm_on_sync else None, self.n_ch, self.buf["l"].ptr)

    def refill(self):
        """every output buffer back to its prefill"""
        for name in self.OUT:
            self.buf[name].refill()

    def read(self, name):
        if name in self.OUT:
            return self.buf[name].get(self.OUT[name], self.shape(name))
        return self.buf[name].get(self.states[name].dtype, self.states[name].shape)

    def free(self):
        for b in self.buf.values():
            b.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()
