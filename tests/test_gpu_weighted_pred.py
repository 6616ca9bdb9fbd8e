"""The ephemeris bank and the prediction and hot hand-over on the device (EXTENSIONS, not in the reference: include/gpsx.h gpsx_wbank,
gpsx_wpred; k_wbank and k_wpred, a wave per receiver each) against their CPU restatements (tests/weighted_pred_ref.py, the rows of
tests/weighted_pred_cases.py, whose predicates tests/test_weighted_pred_reference.py asserts).  The bank: every comparison is for
equality, byte for byte -- the bank and the sync states between canaries, the outputs prefilled; the table at every edge of the PRN
and slot lanes, of the two-records-a-turn copy and of four receivers per workgroup; the merged copy absent, apart and in place.  The
prediction: flags, slots, masks, counts, tx_ms, T and week equal, the doubles within the measured parity bound, all five state arrays
byte for byte (weighted_pred_cases.decisions_clear makes that fair).  Both: host variant = device variant = binding; a second call;
receivers permuted; every refusal with its text; and the stages behind the device chain on weighted_pvt_cases' IF stream."""
import ctypes as C

import numpy as np
import pytest

import weighted_gpu as G
import weighted_pred_cases as PC
import weighted_pred_ref as P
from weighted_gpu import EINVAL, eng  # noqa: F401

pytestmark = pytest.mark.gpu

APART, IN_PLACE, ABSENT = "apart", "in place", "absent"


def _call(eng, la, dev, out=APART, bank=None):
    """gpsx_wbank_dev (dev) or gpsx_wbank on launch `la`: sync states and bank between canaries in device memory, the records and the
    outputs between canaries in device (dev) or host memory, the outputs prefilled -> (rep, merged records or None, bank after)"""
    cfg = P.bank_cfg_record(la.ch)
    prns = np.ascontiguousarray(la.prns, np.uint8)
    sync = PC.sync_states(la)
    bank = la.bank if bank is None else bank
    where = eng if dev else None
    fn = eng.lib.gpsx_wbank_dev if dev else eng.lib.gpsx_wbank
    with G.Pool() as pool:
        d_sync = pool.add(G.Guarded(eng, sync.nbytes, G.STATE_FILL, sync))
        d_bank = pool.add(G.Guarded(eng, bank.nbytes, G.STATE_FILL, bank))
        d_eph = pool.add(G.Guarded(where, la.eph.nbytes, G.STATE_FILL, la.eph))
        d_out = pool.add(G.Guarded(where, la.eph.nbytes))
        d_rep = pool.add(G.Guarded(where, la.n_rx * P.BANK_DTYPE.itemsize))
        p_out = {APART: d_out.ptr, IN_PLACE: d_eph.ptr, ABSENT: None}[out]
        rc = fn(eng.h, cfg.ctypes.data, la.n_rx, la.n_prn, prns.ctypes.data, d_sync.ptr, d_eph.ptr, d_bank.ptr, p_out, d_rep.ptr)
        assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wbank"
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        assert d_sync.untouched()
        if out != IN_PLACE:
            assert d_eph.untouched()
        if out != APART:
            assert d_out.untouched()
        merged = {APART: d_out, IN_PLACE: d_eph, ABSENT: None}[out]
        return (d_rep.get(P.BANK_DTYPE, (la.n_rx,)), None if merged is None else merged.get(P.EPH_DTYPE, (la.n_rx * la.ch,)),
                d_bank.get(P.EPH_DTYPE, (la.n_rx, la.n_prn)))


def _same(got, want, what):
    rep, out, bank = got
    w_rep, w_out, w_bank = want[:3]
    G.same_rows(rep, w_rep, (what, "rep"))
    if out is not None:
        G.same_rows(out, w_out, (what, "merged records"))
    for r in range(len(rep)):
        G.same_rows(bank[r], w_bank[r], (what, "bank of receiver", r))


# ---- 1: the table, byte for byte, at every edge of the launch's shape ------------------------------------------------------------------
# (n_rx, n_prn, ch_per_rx, the merged copy).  Four receivers a workgroup: a second one from 5 on; the PRN and slot lanes end at 64; a
# record is moved by 32 lanes and two a turn, so odd and even numbers of stored entries and of slots meet in the random receivers
SHAPES = [(len(PC.ROWS), PC.N_PRN, PC.CH, APART),      # the canonical shape: what the predicates were proven at
          (len(PC.ROWS), PC.N_PRN, PC.CH, IN_PLACE),
          (len(PC.ROWS), PC.N_PRN, PC.CH, ABSENT),
          (1, 1, 1, APART),
          (3, 31, 4, IN_PLACE),
          (4, 32, 12, APART),
          (5, 33, 63, APART),
          (5, 63, 64, IN_PLACE),
          (67, 64, 12, APART),
          (67, 5, 5, IN_PLACE),
          (21, 64, 64, ABSENT),
          (8, 2, 64, APART)]
SHAPE_IDS = [f"{s[0]}rx-{s[1]}prn-{s[2]}ch-{s[3].replace(' ', '_')}" for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_table_matches_the_restatement(eng, shape):
    n_rx, n_prn, ch, out = shape
    la = PC.launch(n_rx, n_prn, ch)
    want = PC.run(la)
    got = _call(eng, la, True, out)
    _same(got, want, shape)
    if (n_prn, ch) == (PC.N_PRN, PC.CH) and out != ABSENT:
        seen = set()
        for r, row in enumerate(la.rows):          # the predicates, on the DEVICE's bytes
            if row is not None:
                assert row.check(PC.outcome(la, r, got[0], got[1], got[2], want[3])), row.name
                seen.add(row.name)
        assert len(seen) == len(PC.ROWS)


# ---- 2: call equivalences ----------------------------------------------------------------------------------------------------------------
def test_host_variant_device_variant_and_binding_agree(eng):
    from stm32f4_sdr_gps_amd import capi
    la = PC.launch(len(PC.ROWS) + 9, 33, 5)
    want = PC.run(la)
    for out in (APART, IN_PLACE, ABSENT):
        _same(_call(eng, la, True, out), want, ("dev", out))
        _same(_call(eng, la, False, out), want, ("host", out))
    sync = PC.sync_states(la)
    with G.Pool() as pool:
        d_sync = pool.add(G.Guarded(eng, sync.nbytes, G.STATE_FILL, sync))
        for want_out in (True, False):
            d_bank = pool.add(G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank))
            got = eng.wbank(capi.wbank_cfg(la.ch), la.prns, d_sync.ptr.value, la.eph, d_bank.ptr.value, want_out=want_out)
            rep, out = got if want_out else (got, None)
            _same((rep, out, d_bank.get(P.EPH_DTYPE, (la.n_rx, la.n_prn))), want, ("Engine.wbank", want_out))
        assert d_sync.untouched()


def test_a_second_call_refreshes_and_changes_nothing(eng):
    la = PC.launch(40, 33, 12, seed=4)
    first = _call(eng, la, True)
    second = _call(eng, la, True, bank=first[2])
    lb = PC.launch(40, 33, 12, seed=4)
    lb.bank = first[2]
    _same(second, PC.run(lb), "second call")
    assert second[2].tobytes() == first[2].tobytes() and second[1].tobytes() == first[1].tobytes()
    assert second[0]["have_mask"].tobytes() == first[0]["have_mask"].tobytes() and ((second[0]["stored_mask"] & ~first[0]["stored_mask"]) == 0).all()


def test_receivers_permuted_give_the_same_bytes_permuted(eng):
    la, lb = PC.launch(13, 33, 5), PC.launch(13, 33, 5)
    perm = np.random.default_rng(5).permutation(la.n_rx)
    slots = (perm[:, None] * la.ch + np.arange(la.ch)[None, :]).reshape(-1)
    lb.eph, lb.slot_prns, lb.bank = np.ascontiguousarray(la.eph[slots]), np.ascontiguousarray(la.slot_prns[slots]), np.ascontiguousarray(la.bank[perm])
    a, b = _call(eng, la, True), _call(eng, lb, True)
    assert a[0][perm].tobytes() == b[0].tobytes() and a[1][slots].tobytes() == b[1].tobytes() and a[2][perm].tobytes() == b[2].tobytes()


# ---- 3: refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_with_their_text_and_write_nothing(eng):
    """(the last clause of the header's list, a size product that overflows, cannot be reached where a size has 64 bits: n_rx x 64 x
    448 stays below 2^20 x 2^6 x 2^9)"""
    la = PC.launch(6, 5, 4)
    sync = PC.sync_states(la)
    good = dict(null=None, ch=la.ch, reserved=(0, 0, 0), n_rx=la.n_rx, n_prn=la.n_prn, prns=[int(v) for v in la.prns], off={}, out="out")
    by_message = {
        b"null argument": [dict(null=w) for w in ("cfg", "prns", "sync", "eph", "bank", "rep")] + [dict(null="rep", ch=0)],
        b"ch_per_rx must be 1..64": [dict(ch=0), dict(ch=65), dict(ch=-1, reserved=(1, 0, 0))],
        b"reserved must be 0": [dict(reserved=(1, 0, 0)), dict(reserved=(0, -1, 0)), dict(reserved=(0, 0, 7), n_rx=0)],
        b"n_rx must be 1..1048576": [dict(n_rx=0), dict(n_rx=-1), dict(n_rx=(1 << 20) + 1), dict(n_rx=0, n_prn=0)],
        b"n_prn must be 1..64": [dict(n_prn=0), dict(n_prn=65, prns=list(range(1, 66))), dict(n_prn=-3, prns=[0])],
        b"PRN outside 1..210": [dict(prns=[0] + good["prns"][1:]), dict(prns=good["prns"][:-1] + [211]), dict(prns=[255] * la.n_prn, off=dict(bank=8))],
        b"a PRN is listed twice": [dict(prns=good["prns"][:-1] + good["prns"][:1]), dict(prns=[7] * la.n_prn, off=dict(sync=4))],
        b"d_sync_state must be 8-byte aligned": [dict(off=dict(sync=4)), dict(off=dict(sync=1, bank=8))],
        b"d_bank must be 16-byte aligned": [dict(off=dict(bank=8)), dict(off=dict(bank=4, eph=8))],
        b"two arrays overlap (only d_eph_out == d_eph may)": [dict(out=("eph", 256)), dict(out=("eph", -256)), dict(out=("bank", 0)), dict(out=("bank", 512)),
                                                               dict(out=("rep", 0)), dict(out=("sync", 448))],
    }
    dev_only = {b"d_eph, d_eph_out and d_rep must be 16-byte aligned": [dict(off=dict(eph=8)), dict(off=dict(out=8)), dict(off=dict(rep=8))]}
    with G.Pool() as pool:
        d_sync = pool.add(G.Guarded(eng, sync.nbytes, G.STATE_FILL, sync))
        d_bank = pool.add(G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank))
        io = {dev: dict(eph=pool.add(G.Guarded(eng if dev else None, la.eph.nbytes, G.STATE_FILL, la.eph)),
                        out=pool.add(G.Guarded(eng if dev else None, la.eph.nbytes)),
                        rep=pool.add(G.Guarded(eng if dev else None, la.n_rx * P.BANK_DTYPE.itemsize))) for dev in (True, False)}
        fns = {True: eng.lib.gpsx_wbank_dev, False: eng.lib.gpsx_wbank}

        def call(a, dev):
            cfg = P.bank_cfg_record(a["ch"], a["reserved"])
            prns = np.array(a["prns"], np.uint8)
            at = dict(sync=d_sync, bank=d_bank, **io[dev])

            def ptr(name):
                return None if a["null"] == name else C.c_void_p(at[name].ptr.value + a["off"].get(name, 0))
            p_out = ptr("out") if a["out"] == "out" else C.c_void_p(at[a["out"][0]].ptr.value + a["out"][1])
            return fns[dev](eng.h, None if a["null"] == "cfg" else cfg.ctypes.data, a["n_rx"], a["n_prn"], None if a["null"] == "prns" else prns.ctypes.data,
                            ptr("sync"), ptr("eph"), ptr("bank"), p_out, ptr("rep"))
        bufs = [d_sync, d_bank, *io[True].values(), *io[False].values()]
        G.refusals(eng, by_message, good, call, bufs)
        for message, changes in dev_only.items():
            for change in changes:
                for b in bufs:
                    b.refill()
                assert call({**good, **change}, True) == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (change, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()
                assert all(b.untouched() for b in bufs), change
        # the context still works, and the limits themselves are accepted: d_eph_out NULL, d_eph itself, and an array that ends where the next begins
        want = PC.run(la)
        for change in (dict(out=("eph", 0)), dict(null="out")):
            for dev in (False, True):
                for b in bufs:
                    b.refill()
                assert call({**good, **change}, dev) == 0, (change, eng.lib.gpsx_last_error(eng.h))
                assert eng.lib.gpsx_synchronize(eng.h) == 0
                G.same_rows(io[dev]["rep"].get(P.BANK_DTYPE, (la.n_rx,)), want[0], (change, dev))
                assert d_bank.get(P.EPH_DTYPE, (la.n_rx, la.n_prn)).tobytes() == want[2].tobytes()


# ---- 4: behind the device stages: a slot that lost its ephemeris keeps its place in the fix -----------------------------------------------
def test_behind_the_device_stages_a_lost_ephemeris_comes_from_the_bank(eng):
    """weighted_pvt_cases' stream (four orbiting satellites, 25 000 blocks, MOVING gains) through the device stages in
    weighted_pvt_cases.LAUNCHES with gpsx_wbank_dev behind gpsx_weph_dev on the arrays where they lie, the list holding the four PRNs
    among others: after every launch the report, the bank and the merged records equal the restatement's on the device's own records
    and the bank as the launch before left it.  At block 24 576 slot 2's ephemeris state is cleared, as a hand-over clears it; 424
    blocks rebuild no ephemeris, so its own record of the last launch lacks VALID.  Then from_bank_mask is bit 2 alone, the merged
    record is the bank's byte for byte, gpsx_wfix_dev finds no fix on the launch's own records (three satellites) and on the merged
    records the very fix, byte for byte, that it finds on the records of the state that was not cleared (gpsx_weph_dev once more on the
    same words with the saved state).  Cost: the stream's synthesis (about 25 s of CPU, cached per process in
    weighted_pvt_cases._memo) and its upload, plus a few seconds of GPU."""
    import weighted_fix_ref as F
    import weighted_kf_cases as K
    import weighted_pvt_cases as S
    lib, n_ch = eng.lib, 4
    prns = np.array([31, S.PRNS[2], S.PRNS[0], 2, S.PRNS[3], S.PRNS[1], 210], np.uint8)      # (the stream's are 1, 3, 4, 5)
    assert len(set(int(q) for q in prns)) == len(prns)
    blocks = S.blocks()
    d_if = eng.malloc(blocks.nbytes)
    eng.h2d(d_if, blocks)
    chain = G.Chain(eng, S.sync_cfg_dev(S.MOVING), dict(S.fresh_states(), sync=S.handover()), max(S.LAUNCHES), S.MAX_BAD_WORDS, S.EDGE_GUARD)
    fcfg, cfg = K.if_cfgs()[0], P.bank_cfg_record(n_ch)
    bank0 = P.empty_bank(1, len(prns))
    bufs = dict(bank=G.Guarded(eng, bank0.nbytes, G.STATE_FILL, bank0), out=G.Guarded(eng, n_ch * 256), rep=G.Guarded(eng, 32),
                fix=G.Guarded(eng, 3 * F.FIX_DTYPE.itemsize))

    def wfix(d_eph, k):
        eng._chk(lib.gpsx_wfix_dev(eng.h, fcfg.ctypes.data, chain.buf["o"].ptr, d_eph, None, None, 1, C.c_void_p(bufs["fix"].ptr.value + k * F.FIX_DTYPE.itemsize),
                                   None), "gpsx_wfix_dev")
    try:
        at, bank, saved = 0, bank0, None
        for k, n in enumerate(S.LAUNCHES):
            last = k == len(S.LAUNCHES) - 1
            if last:
                saved = chain.read("eph")
                cleared = saved.copy()
                cleared[2] = np.zeros(1, saved.dtype)[0]
                chain.buf["eph"].put(cleared)
            chain.sync(d_if + at * 4092, n)
            chain.words()
            chain.obs()
            chain.eph()
            for name in ("out", "rep"):
                bufs[name].refill()
            eng._chk(lib.gpsx_wbank_dev(eng.h, cfg.ctypes.data, 1, len(prns), prns.ctypes.data, chain.buf["sync"].ptr, chain.buf["e"].ptr, bufs["bank"].ptr,
                                        bufs["out"].ptr, bufs["rep"].ptr), "gpsx_wbank_dev")
            assert lib.gpsx_last_kernel(eng.h) == b"k_wbank"
            eng.synchronize()
            at += n
            eph, slots = chain.read("e"), chain.read("sync")["loop"]["prn"]
            assert [int(v) for v in slots] == list(S.PRNS)
            rep, out = bufs["rep"].get(P.BANK_DTYPE, (1,)), bufs["out"].get(P.EPH_DTYPE, (n_ch,))
            w_rep, w_out = P.bank(n_ch, prns, slots, eph, bank)          # (advances `bank`, the restatement's, in place)
            _same((rep, out, bufs["bank"].get(P.EPH_DTYPE, (1, len(prns)))), (w_rep, w_out, bank), ("launch", k))
            print("launch", k, "own VALID", [int(f) & P.F_VALID for f in eph["flags"]], "stored", bin(int(rep["stored_mask"][0])), "have",
                  bin(int(rep["have_mask"][0])), "from the bank", bin(int(rep["from_bank_mask"][0])))
            if k == len(S.LAUNCHES) - 2:
                assert int(rep["n_have"][0]) == 4, "the four ephemerides are decoded before block 24 576"
        index = [list(prns).index(q) for q in S.PRNS]
        assert not int(eph["flags"][2]) & P.F_VALID and int(rep["from_bank_mask"][0]) == 4 and int(rep["have_mask"][0]) == sum(1 << p for p in index)
        assert out[2].tobytes() == bank[0, index[2]].tobytes() and int(out[2]["flags"]) == P.F_VALID
        assert all(out[j].tobytes() == eph[j].tobytes() and int(eph[j]["flags"]) & P.F_VALID for j in (0, 1, 3))
        wfix(chain.buf["e"].ptr, 0)
        wfix(bufs["out"].ptr, 1)
        chain.buf["eph"].put(saved)
        chain.eph()                                                    # the same words on the state that was not cleared
        wfix(chain.buf["e"].ptr, 2)
        eng.synchronize()
        own, merged, whole = bufs["fix"].get(F.FIX_DTYPE, (3,))
        assert int(chain.read("e")["flags"][2]) & P.F_VALID
        print("fix on the launch's own records", int(own["flags"]), int(own["n_used"]), "on the merged records", int(merged["flags"]), int(merged["n_used"]),
              "position error", float(np.linalg.norm(merged["rr"] - S.RX)))
        assert not int(own["flags"]) & F.F_FIX and int(merged["flags"]) == F.F_FIX and int(merged["n_used"]) == 4
        assert merged.tobytes() == whole.tobytes()
    finally:
        for b in bufs.values():
            b.free()
        chain.free()
        eng.free(d_if)


# ==== gpsx_wpred: prediction and hot hand-over =================================================================================================
NAMES = ("sync", "lock", "nav", "obs", "eph")


def _pcall(eng, la, cfg, dev, nulls=(), want_pred=True, states=None):
    """gpsx_wpred_dev (dev) or gpsx_wpred on launch `la`: the filter states, the bank and the five state arrays (those named in `nulls`: a
    NULL pointer) between canaries in device memory, the outputs between canaries, prefilled -> (rx, pred or None, {name: states after})"""
    states = la.states if states is None else states
    prns = np.ascontiguousarray(la.prns, np.uint8)
    where = eng if dev else None
    fn = eng.lib.gpsx_wpred_dev if dev else eng.lib.gpsx_wpred
    with G.Pool() as pool:
        st = {k: None if k in nulls else pool.add(G.Guarded(eng, states[k].nbytes, G.STATE_FILL, states[k])) for k in NAMES}
        d_kf = pool.add(G.Guarded(eng, la.kf.nbytes, G.STATE_FILL, la.kf))
        d_bank = pool.add(G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank))
        d_rx = pool.add(G.Guarded(where, la.n_rx * P.PRED_RX_DTYPE.itemsize))
        d_pred = pool.add(G.Guarded(where, la.n_rx * la.n_prn * P.PRED_DTYPE.itemsize))
        rc = fn(eng.h, cfg.ctypes.data, la.n_rx, la.n_prn, prns.ctypes.data, d_kf.ptr, d_bank.ptr, *[None if st[k] is None else st[k].ptr for k in NAMES],
                d_rx.ptr, d_pred.ptr if want_pred else None)
        assert rc == 0, (rc, eng.lib.gpsx_last_error(eng.h))
        assert eng.lib.gpsx_last_kernel(eng.h) == b"k_wpred"
        assert eng.lib.gpsx_synchronize(eng.h) == 0
        assert d_kf.untouched() and d_bank.untouched()
        if not want_pred:
            assert d_pred.untouched()
        return (d_rx.get(P.PRED_RX_DTYPE, (la.n_rx,)), d_pred.get(P.PRED_DTYPE, (la.n_rx, la.n_prn)) if want_pred else None,
                {k: None if st[k] is None else st[k].get(states[k].dtype, states[k].shape) for k in NAMES})


def _psame(la, cfg, got, want, what, label=None):
    """records within the parity bound (integers equal), all five state arrays byte for byte -- which the clearance makes fair"""
    assert PC.decisions_clear(la, cfg, want[1], want[3]) == [], "a receiver of the table does not stand clear of the parity bound"
    if got[1] is not None:
        PC.compare(got[0], got[1], want[0], want[1], float(cfg["mps_per_hz"][0]), label=label)
    else:
        assert got[0].tobytes() == want[0].tobytes(), what
    for k in NAMES:
        if want[2][k] is not None:
            G.same_rows(got[2][k], want[2][k], (what, k))


# (n_rx, n_prn, ch_per_rx, NULL state arrays, handover, evict_after_blocks or None: the table's)
PSHAPES = [(len(PC.PRED_ROWS), PC.P_N_PRN, PC.P_CH, (), 1, None),      # the canonical shape: what the predicates were proven at
           (len(PC.PRED_ROWS), PC.P_N_PRN, PC.P_CH, (), 0, None),
           (1, 1, 1, (), 1, None),
           (3, 31, 4, ("nav",), 1, None),
           (4, 32, 12, ("obs",), 1, None),
           (5, 33, 63, ("eph",), 0, None),
           (5, 63, 64, (), 1, None),
           (67, 64, 12, ("nav", "obs", "eph"), 1, None),
           (21, 12, 64, ("lock",), 1, 0),
           (67, 10, 6, ("lock", "nav", "obs", "eph"), 1, 0)]
PSHAPE_IDS = [f"{s[0]}rx-{s[1]}prn-{s[2]}ch-handover{s[4]}" + ("-no_" + "_".join(s[3]) if s[3] else "") for s in PSHAPES]


@pytest.mark.parametrize("shape", PSHAPES, ids=PSHAPE_IDS)
def test_the_prediction_table_matches_the_restatement(eng, shape):
    n_rx, n_prn, ch, nulls, handover, evict = shape
    la = PC.pred_launch(n_rx, n_prn, ch)
    cfg = PC.pred_cfg(ch, handover, **({} if evict is None else dict(evict_after_blocks=evict)))
    want = PC.pred_run(la, cfg, nulls)
    got = _pcall(eng, la, cfg, True, nulls)
    _psame(la, cfg, got, want, shape, label=PSHAPE_IDS[PSHAPES.index(shape)])
    for r, t in enumerate(want[3]):          # what the definition leaves alone: a slot that is not written keeps every byte in all five arrays
        for j in range(ch):
            if t["kind"] != "run" or j not in t["written"]:
                for k in NAMES:
                    if k not in nulls:
                        assert got[2][k][r * ch + j].tobytes() == la.states[k][r * ch + j].tobytes(), (shape, r, j, k)
    if handover == 0:
        assert all(got[2][k].tobytes() == la.states[k].tobytes() for k in NAMES if k not in nulls)
        assert not (got[1]["flags"] & (P.P_ASSIGNED | P.P_DROPPED)).any() and not got[0]["assigned_mask"].any()
    if (n_prn, ch, handover) == (PC.P_N_PRN, PC.P_CH, 1) and not nulls:
        for r, row in enumerate(la.rows):          # the predicates, on the DEVICE's bytes (the trace is the restatement's)
            assert row.check(PC.pred_outcome(la, r, got[0], got[1], got[2], want[3])), row.name


def test_prediction_host_variant_device_variant_and_binding_agree(eng):
    la = PC.pred_launch(len(PC.PRED_ROWS) + 5, 12, 7)
    cfg = PC.pred_cfg(7)
    want = PC.pred_run(la, cfg)
    dev = _pcall(eng, la, cfg, True)
    host = _pcall(eng, la, cfg, False)
    _psame(la, cfg, dev, want, "dev")
    assert host[0].tobytes() == dev[0].tobytes() and host[1].tobytes() == dev[1].tobytes() and all(host[2][k].tobytes() == dev[2][k].tobytes() for k in NAMES)
    for variant in (True, False):
        none = _pcall(eng, la, cfg, variant, want_pred=False)
        assert none[1] is None and none[0].tobytes() == dev[0].tobytes() and all(none[2][k].tobytes() == dev[2][k].tobytes() for k in NAMES)
    with G.Pool() as pool:
        st = {k: pool.add(G.Guarded(eng, la.states[k].nbytes, G.STATE_FILL, la.states[k])) for k in NAMES}
        d_kf, d_bank = pool.add(G.Guarded(eng, la.kf.nbytes, G.STATE_FILL, la.kf)), pool.add(G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank))
        rx, pred = eng.wpred(cfg, la.prns, la.n_rx, d_kf.ptr.value, d_bank.ptr.value, *[st[k].ptr.value for k in NAMES])
        assert rx.tobytes() == dev[0].tobytes() and pred.tobytes() == dev[1].tobytes()
        assert all(st[k].get(la.states[k].dtype, la.states[k].shape).tobytes() == dev[2][k].tobytes() for k in NAMES)


def test_a_second_prediction_tracks_what_the_first_handed_over_and_writes_nothing(eng):
    la = PC.pred_launch(len(PC.PRED_ROWS) + 9, 12, 7)
    cfg = PC.pred_cfg(7, evict_after_blocks=0)
    first = _pcall(eng, la, cfg, True)
    second = _pcall(eng, la, cfg, True, states=first[2])
    for k in NAMES:
        assert second[2][k].tobytes() == first[2][k].tobytes(), k
    assert not second[0]["n_assigned"].any() and not second[0]["assigned_mask"].any()
    held = (first[1]["flags"] & (P.P_ASSIGNED | P.P_TRACKED)) != 0
    assert held.any() and ((second[1]["flags"][held] & P.P_TRACKED) != 0).all() and ((second[1]["flags"][held] & P.P_ASSIGNED) == 0).all()
    for f in ("pr_m", "code_phase", "f_hz", "el", "az", "tx_ms"):
        assert second[1][f].tobytes() == first[1][f].tobytes(), f


def test_prediction_receivers_permuted_give_the_same_bytes_permuted(eng):
    la, lb = PC.pred_launch(13, 12, 5, clear=False), PC.pred_launch(13, 12, 5, clear=False)
    perm = np.random.default_rng(5).permutation(la.n_rx)
    slots = (perm[:, None] * la.ch + np.arange(la.ch)[None, :]).reshape(-1)
    lb.kf, lb.bank, lb.states = np.ascontiguousarray(la.kf[perm]), np.ascontiguousarray(la.bank[perm]), {k: np.ascontiguousarray(v[slots]) for k, v in la.states.items()}
    cfg = PC.pred_cfg(5)
    a, b = _pcall(eng, la, cfg, True), _pcall(eng, lb, cfg, True)
    assert a[0][perm].tobytes() == b[0].tobytes() and a[1][perm].tobytes() == b[1].tobytes()
    for k in NAMES:
        assert a[2][k][slots].tobytes() == b[2][k].tobytes(), k


def test_prediction_refusals_come_with_their_text_and_write_nothing(eng):
    la = PC.pred_launch(3)
    nan, inf = float("nan"), float("inf")
    good = dict(null=None, ion0=0.0, mps=float(PC.VR.L1CA_WLOOP), el_min=0.1, sig=(30.0, 2.0), ch=la.ch, lead=7, evict=PC.EVICT, handover=1, reserved=0,
                n_rx=la.n_rx, n_prn=la.n_prn, prns=[int(v) for v in la.prns], off={})
    by_message = {
        b"null argument": [dict(null=w) for w in ("cfg", "prns", "kf", "bank", "sync", "rx")] + [dict(null="rx", ch=0)],
        b"an ionosphere coefficient is not finite": [dict(ion0=nan), dict(ion0=inf, mps=0.0)],
        b"mps_per_hz must be finite and not 0": [dict(mps=0.0), dict(mps=nan), dict(mps=-inf, el_min=9.0)],
        b"el_min_rad must be finite and within -pi/2..pi/2": [dict(el_min=nan), dict(el_min=1.5708), dict(el_min=-inf, sig=(0.0, 1.0))],
        b"max_sigma_m and max_sigma_hz must be finite and above 0": [dict(sig=(0.0, 1.0)), dict(sig=(1.0, -1.0)), dict(sig=(nan, 1.0)), dict(sig=(1.0, inf), ch=0)],
        b"ch_per_rx must be 1..64": [dict(ch=0), dict(ch=65), dict(ch=-1, lead=-1)],
        b"lead_blocks must be 0..4096": [dict(lead=-1), dict(lead=4097, evict=-1)],
        b"evict_after_blocks must be 0..1073741824": [dict(evict=-1), dict(evict=(1 << 30) + 1, handover=2)],
        b"handover must be 0 or 1": [dict(handover=2), dict(handover=-1, reserved=1)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1, null="lock")],
        b"evict_after_blocks needs d_lock_state": [dict(null="lock"), dict(null="lock", evict=1, n_rx=0)],
        b"n_rx must be 1..1048576": [dict(n_rx=0), dict(n_rx=(1 << 20) + 1, n_prn=0)],
        b"n_prn must be 1..64": [dict(n_prn=0), dict(n_prn=65, prns=list(range(1, 66)))],
        b"PRN outside 1..210": [dict(prns=[0] + good["prns"][1:]), dict(prns=good["prns"][:-1] + [211])],
        b"a PRN is listed twice": [dict(prns=good["prns"][:-1] + good["prns"][:1]), dict(prns=[7] * la.n_prn, off=dict(kf=8))],
        b"d_kf_state and d_bank must be 16-byte aligned": [dict(off=dict(kf=8)), dict(off=dict(bank=8, rx=8))],
    }
    dev_only = {b"d_rx and d_pred must be 16-byte aligned": [dict(off=dict(rx=8)), dict(off=dict(pred=8))]}
    with G.Pool() as pool:
        st = {k: pool.add(G.Guarded(eng, la.states[k].nbytes, G.STATE_FILL, la.states[k])) for k in NAMES}
        fixed = dict(kf=pool.add(G.Guarded(eng, la.kf.nbytes, G.STATE_FILL, la.kf)), bank=pool.add(G.Guarded(eng, la.bank.nbytes, G.STATE_FILL, la.bank)))
        outs = {dev: dict(rx=pool.add(G.Guarded(eng if dev else None, la.n_rx * 64)), pred=pool.add(G.Guarded(eng if dev else None, la.n_rx * la.n_prn * 64)))
                for dev in (True, False)}
        fns = {True: eng.lib.gpsx_wpred_dev, False: eng.lib.gpsx_wpred}

        def call(a, dev):
            cfg = P.pred_cfg(a["ch"], a["mps"], a["el_min"], a["sig"][0], a["sig"][1], a["lead"], a["evict"], a["handover"])
            cfg["ion"][0, 3], cfg["reserved"][0, 2] = a["ion0"], a["reserved"]
            prns = np.array(a["prns"], np.uint8)
            at = dict(st, **fixed, **outs[dev])

            def ptr(name):
                return None if a["null"] == name else C.c_void_p(at[name].ptr.value + a["off"].get(name, 0))
            return fns[dev](eng.h, None if a["null"] == "cfg" else cfg.ctypes.data, a["n_rx"], a["n_prn"], None if a["null"] == "prns" else prns.ctypes.data,
                            ptr("kf"), ptr("bank"), *[ptr(k) for k in NAMES], ptr("rx"), ptr("pred"))
        bufs = [*st.values(), *fixed.values(), *outs[True].values(), *outs[False].values()]
        G.refusals(eng, by_message, good, call, bufs)
        for message, changes in dev_only.items():
            for change in changes:
                for b in bufs:
                    b.refill()
                assert call({**good, **change}, True) == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (change, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()
                assert all(b.untouched() for b in bufs), change
        for change in (dict(lead=4096), dict(lead=0, evict=1 << 30), dict(el_min=-1.5707963267948966), dict(handover=0, null="pred")):
            for dev in (False, True):
                assert call({**good, **change}, dev) == 0, (change, eng.lib.gpsx_last_error(eng.h))
                assert eng.lib.gpsx_synchronize(eng.h) == 0


def test_behind_the_device_stages_prediction_and_hot_re_acquisition(eng):
    """weighted_pvt_cases' stream through weighted_gpu.Chain with gpsx_wbank_dev, gpsx_wfix_dev, gpsx_wvel_dev and gpsx_wkf_dev (on the
    merged records) after every launch.  At block 24 576 gpsx_wpred_dev on the arrays where they lie: its records equal the restatement's
    on the device's own filter state and bank, and the predicted transmit times and frequencies are within 1.5 x
    weighted_pred_cases.MEASURED of the synthesiser's truth.  The states are copied to a second set of buffers, slot 2 is emptied there
    and gpsx_wpred_dev with handover = 1 hands PRN 4 back to it; both sets run the last 424 blocks: slot 2's final phase and frequency
    are within 1.5 x MEASURED's repull figures of the undisturbed set's, from_bank_mask has bit 2 and its merged record is the bank's.
    Cost: the stream's synthesis (about 25 s of CPU, cached per process) and its upload, plus a few seconds of GPU."""
    import weighted_acq_ref as Q
    import weighted_fix_ref as F
    import weighted_kf_ref as R
    import weighted_pvt_cases as S
    import weighted_vel_ref as V
    lib, n_ch, prns = eng.lib, 4, np.array(PC.STREAM_PRNS, np.uint8)
    blocks = S.blocks()
    d_if = eng.malloc(blocks.nbytes)
    eng.h2d(d_if, blocks)
    fcfg, vcfg, kcfg = PC.stream_filter_cfgs()
    bcfg = P.bank_cfg_record(n_ch)
    bank0 = P.empty_bank(1, len(prns))
    a = G.Chain(eng, S.sync_cfg_dev(S.MOVING), dict(S.fresh_states(), sync=S.handover()), max(S.LAUNCHES), S.MAX_BAD_WORDS, S.EDGE_GUARD)
    b = None
    bufs = dict(bank=G.Guarded(eng, bank0.nbytes, G.STATE_FILL, bank0), out=G.Guarded(eng, n_ch * 256), rep=G.Guarded(eng, 32), fix=G.Guarded(eng, F.FIX_DTYPE.itemsize),
                vel=G.Guarded(eng, V.VEL_DTYPE.itemsize), kf=G.Guarded(eng, R.KF_DTYPE.itemsize), state=G.Guarded(eng, 384, G.STATE_FILL, np.zeros(1, R.STATE_DTYPE)),
                rx=G.Guarded(eng, 64), pred=G.Guarded(eng, len(prns) * 64), bank_b=G.Guarded(eng, bank0.nbytes, G.STATE_FILL, bank0), out_b=G.Guarded(eng, n_ch * 256),
                rep_b=G.Guarded(eng, 32))

    def launch(chain, at, n, bank, out, rep):
        chain.sync(d_if + at * 4092, n)
        chain.words()
        chain.obs()
        chain.eph()
        eng._chk(lib.gpsx_wbank_dev(eng.h, bcfg.ctypes.data, 1, len(prns), prns.ctypes.data, chain.buf["sync"].ptr, chain.buf["e"].ptr, bufs[bank].ptr, bufs[out].ptr,
                                    bufs[rep].ptr), "gpsx_wbank_dev")

    def wpred(cfg, chain, nulls=False):
        for name in ("rx", "pred"):
            bufs[name].refill()
        st = [chain.buf["sync"].ptr] + [None] * 4 if nulls else [chain.buf["sync"].ptr, None, chain.buf["nav"].ptr, chain.buf["obs"].ptr, chain.buf["eph"].ptr]
        eng._chk(lib.gpsx_wpred_dev(eng.h, cfg.ctypes.data, 1, len(prns), prns.ctypes.data, bufs["state"].ptr, bufs["bank"].ptr, *st, bufs["rx"].ptr, bufs["pred"].ptr),
                 "gpsx_wpred_dev")
        assert lib.gpsx_last_kernel(eng.h) == b"k_wpred"
        eng.synchronize()
        return bufs["rx"].get(P.PRED_RX_DTYPE, (1,)), bufs["pred"].get(P.PRED_DTYPE, (1, len(prns)))
    try:
        at, flags = 0, []
        for k, n in enumerate(S.LAUNCHES[:-1]):
            launch(a, at, n, "bank", "out", "rep")
            eng._chk(lib.gpsx_wfix_dev(eng.h, fcfg.ctypes.data, a.buf["o"].ptr, bufs["out"].ptr, None, bufs["fix"].ptr if at else None, 1, bufs["fix"].ptr, None), "wfix")
            eng._chk(lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, a.buf["o"].ptr, bufs["out"].ptr, None, bufs["fix"].ptr, 1, bufs["vel"].ptr), "wvel")
            eng._chk(lib.gpsx_wkf_dev(eng.h, kcfg.ctypes.data, a.buf["o"].ptr, bufs["out"].ptr, None, bufs["fix"].ptr, bufs["vel"].ptr, 1, n, bufs["state"].ptr,
                                      bufs["kf"].ptr), "wkf")
            eng.synchronize()
            at += n
            flags.append(int(bufs["kf"].get(R.KF_DTYPE, 1)["flags"][0]))
        assert at == 24576 and flags[-1] == R.F_INIT, flags
        # -- the prediction on the device's own arrays
        state, bank = bufs["state"].get(R.STATE_DTYPE, (1,)), bufs["bank"].get(P.EPH_DTYPE, (1, len(prns)))
        rx, pred = wpred(PC.stream_cfg(0), a)
        sync_now = a.read("sync")
        w_rx, w_pred = P.predict(PC.stream_cfg(0), prns, state, bank, sync_now.copy())
        print("parity", PC.compare(rx, pred, w_rx, w_pred, float(V.L1CA_WLOOP), label="from IF samples"))
        assert a.read("sync").tobytes() == sync_now.tobytes() and int(rx["n_tracked"][0]) == 4 and int(rx["n_visible"][0]) == 4
        d_phase, d_freq, block = PC.prediction_errors(pred[0], rx["t_ms"][0])
        print("prediction errors at block", block, d_phase, "samples", d_freq, "Hz")
        assert block == 24576 and np.abs(d_phase).max() <= 1.5 * PC.MEASURED["pred_phase_samples"] and np.abs(d_freq).max() <= 1.5 * PC.MEASURED["pred_freq_hz"]
        # -- a second set of buffers with slot 2 emptied, the hot hand-over
        st_b = {name: a.read(name) for name in ("sync", "nav", "obs", "eph")}
        st_b["sync"][2] = Q.handover_state(P.PRN_NONE)
        for name in ("nav", "obs", "eph"):
            st_b[name][2] = np.zeros(1, st_b[name].dtype)[0]
        b = G.Chain(eng, S.sync_cfg_dev(S.MOVING), st_b, max(S.LAUNCHES), S.MAX_BAD_WORDS, S.EDGE_GUARD)
        bufs["bank_b"].put(bank)
        rx, pred = wpred(PC.stream_cfg(1), b)
        p4 = PC.STREAM_PRNS.index(S.PRNS[2])
        assert int(rx["assigned_mask"][0]) == 4 and int(pred[0, p4]["slot"]) == 2 and int(rx["n_tracked"][0]) == 3
        handed = b.read("sync")[2]["loop"]
        assert int(handed["prn"]) == S.PRNS[2] and float(handed["code_phase_fine"]) == float(np.float32(pred[0, p4]["code_phase"])) and \
            float(handed["if_freq_offset_hz"]) == float(np.float32(pred[0, p4]["f_hz"]))
        n = S.LAUNCHES[-1]
        launch(a, at, n, "bank", "out", "rep")
        launch(b, at, n, "bank_b", "out_b", "rep_b")
        eng.synchronize()
        und, got = a.read("sync")[2]["loop"], b.read("sync")[2]["loop"]
        d_phase = (float(got["code_phase_fine"]) - float(und["code_phase_fine"]) + 8184.0) % 16368.0 - 8184.0
        d_freq = float(got["if_freq_offset_hz"]) - float(und["if_freq_offset_hz"])
        print("slot 2 after 424 blocks against the undisturbed set:", d_phase, "samples", d_freq, "Hz")
        assert abs(d_phase) <= 1.5 * PC.MEASURED["repull_phase_samples"] and abs(d_freq) <= 1.5 * PC.MEASURED["repull_freq_hz"]
        rep_b, out_b, own = bufs["rep_b"].get(P.BANK_DTYPE, (1,)), bufs["out_b"].get(P.EPH_DTYPE, (n_ch,)), b.read("e")
        assert int(rep_b["from_bank_mask"][0]) & 4 and not int(own["flags"][2]) & P.F_VALID
        assert out_b[2].tobytes() == bufs["bank_b"].get(P.EPH_DTYPE, (1, len(prns)))[0, p4].tobytes()
    finally:
        for buf in bufs.values():
            buf.free()
        a.free()
        if b is not None:
            b.free()
        eng.free(d_if)
