"""The time-of-week aiding on the device (include/gpsx.h gpsx_wtow, csrc/k_wtow.hip) against its restatement (tests/weighted_tow_ref.py)
on the fabricated receivers of tests/weighted_tow_cases.py: both record arrays, the observable states, the sync states and the
observables between canaries, byte for byte, untouched slots included -- every decision is exact, so there is no tolerance anywhere;
the predicates on the device's bytes; host variant = device variant = binding; a second call; receivers permuted; every refusal with
its text; and, behind weighted_gpu.Chain on weighted_pvt_cases' IF stream, both call orders."""
import ctypes as C
import itertools

import numpy as np
import pytest

import weighted_gpu as G
import weighted_obs_ref as O
import weighted_pred_cases as PC
import weighted_pred_ref as P
import weighted_tow_cases as TC
import weighted_tow_ref as T
from weighted_gpu import eng  # noqa: F401  (the module's engine fixture)

pytestmark = pytest.mark.gpu
EINVAL = G.EINVAL


def _call(eng, la, cfg, dev, with_obs=True, arrays=None):
    """gpsx_wtow_dev (dev) or gpsx_wtow on launch `la` through weighted_gpu.run_stage: the sync states, the observable states and the
    observables as its states (between canaries, read back whole), the prediction's records as its inputs, both record arrays in one
    prefilled output buffer between canaries -> (tow, tow_rx, sync after, states after, obs after or None)"""
    sync, states, obs = arrays or (la.sync, la.states, la.obs)
    prns = np.ascontiguousarray(la.prns, np.uint8)
    fn = eng.lib.gpsx_wtow_dev if dev else eng.lib.gpsx_wtow
    n_ch = la.n_rx * la.ch
    tow_bytes = n_ch * T.TOW_DTYPE.itemsize

    def call(p_in, p_st, p_out, k):
        return fn(eng.h, cfg.ctypes.data, la.n_rx, la.n_prn, prns.ctypes.data, p_in[0], p_in[1], p_st[0], p_st[1], p_st[2], p_out,
                  C.c_void_p(p_out.value + tow_bytes))
    outs, after, codes = G.run_stage(eng, call, b"k_wtow", [sync, states, obs if with_obs else None],
                                     [([la.pred_rx, la.pred], np.uint8, (tow_bytes + la.n_rx * T.TOW_RX_DTYPE.itemsize,))], dev=dev)
    assert codes == [0]
    return outs[0][:tow_bytes].view(T.TOW_DTYPE), outs[0][tow_bytes:].view(T.TOW_RX_DTYPE), after[0], after[1], after[2]


def _same(got, want, what):
    for g, w, name in zip(got, want, ("tow", "tow_rx", "sync", "states", "obs")):
        if w is None:
            assert g is None, (what, name)
        elif name == "tow_rx":
            assert g.tobytes() == w.tobytes(), (what, name, [r for r in range(len(w)) if g[r].tobytes() != w[r].tobytes()][:4])
        else:
            G.same_rows(g, w, (what, name))


# (n_rx, n_prn, ch_per_rx, resolve, rearm, d_obs present): n_rx 1, 4, 5 (a second workgroup) and 67; ch_per_rx 1, 4, 33 and 64; n_prn 1, 12, 63 and 64
N_ROWS = len(TC.ROWS)
SHAPES = [(N_ROWS, TC.N_PRN, TC.CH, resolve, rearm, with_obs) for (resolve, rearm), with_obs in zip(itertools.product((0, 1), (0, 1)), (True, False, False, True))] + \
         [(N_ROWS, TC.N_PRN, TC.CH, 1, 1, False), (N_ROWS, TC.N_PRN, TC.CH, 0, 0, False),
          (1, 1, 1, 1, 0, True), (4, 12, 4, 1, 1, True), (5, 63, 33, 0, 1, False), (5, 64, 64, 1, 1, True), (67, 12, 33, 1, 0, True), (67, 64, 1, 0, 0, True),
          (N_ROWS + 9, 12, 7, 1, 1, True)]
SHAPE_IDS = [f"{s[0]}rx-{s[1]}prn-{s[2]}ch-resolve{s[3]}-rearm{s[4]}" + ("" if s[5] else "-no_obs") for s in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_the_table_matches_the_restatement(eng, shape):
    n_rx, n_prn, ch, resolve, rearm, with_obs = shape
    la = TC.launch(n_rx, n_prn, ch)
    cfg = TC.cfg(ch, resolve, rearm)
    want = TC.run(la, cfg, with_obs)
    got = _call(eng, la, cfg, True, with_obs)
    _same(got, want, shape)
    flags = want[0]["flags"]
    for at in range(n_rx * ch):      # what the definition leaves alone: said of the device's bytes, not through the restatement's
        f = int(flags[at])
        if not f & (T.T_AIDED | T.T_AGREES):
            assert got[3][at].tobytes() == la.states[at].tobytes() and (not with_obs or got[4][at].tobytes() == la.obs[at].tobytes()), (shape, at)
        if not f & T.T_REARMED:
            assert got[2][at].tobytes() == la.sync[at].tobytes(), (shape, at)
    if (n_prn, ch) == (TC.N_PRN, TC.CH):
        for r, row in enumerate(la.rows):          # the predicates, on the DEVICE's bytes
            assert row.check(TC.outcome(la, r, cfg, *got)), (row.name, shape)


def test_host_variant_device_variant_and_binding_agree(eng):
    la = TC.launch(N_ROWS + 5, 12, 7)
    cfg = TC.cfg(7, 1, 1)
    want = TC.run(la, cfg)
    dev = _call(eng, la, cfg, True)
    host = _call(eng, la, cfg, False)
    _same(dev, want, "dev")
    _same(host, dev, "host")
    for variant in (True, False):
        none = _call(eng, la, cfg, variant, with_obs=False)
        assert none[4] is None and all(none[k].tobytes() == dev[k].tobytes() for k in range(4))
    from stm32f4_sdr_gps_amd import capi
    assert capi.wtow_cfg(7, TC.MAX_SIGMA, TC.MAX_RESID, TC.MAX_AGE, 1, 1).tobytes() == cfg.tobytes()
    with G.Pool() as pool:
        bufs = [pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for a in (la.pred_rx, la.pred, la.sync, la.states, la.obs)]
        tow, tow_rx = eng.wtow(cfg, la.prns, la.n_rx, *[b.ptr.value for b in bufs])
        assert tow.tobytes() == dev[0].tobytes() and tow_rx.tobytes() == dev[1].tobytes() and bufs[0].untouched() and bufs[1].untouched()
        assert all(b.get(a.dtype, a.shape).tobytes() == d.tobytes() for b, a, d in zip(bufs[2:], (la.sync, la.states, la.obs), dev[2:]))
        # ... and the binding's _dev form on the result: the records in device memory
        d_tow, d_tow_rx = pool.add(G.Guarded(eng, tow.nbytes)), pool.add(G.Guarded(eng, tow_rx.nbytes))
        eng.wtow_dev(cfg, la.prns, la.n_rx, *[b.ptr.value for b in bufs], d_tow.ptr.value, d_tow_rx.ptr.value)
        eng.synchronize()
        again = d_tow.get(T.TOW_DTYPE, tow.shape)
        assert not (again["flags"] & T.T_AIDED).any() and ((again["flags"][(tow["flags"] & T.T_AIDED) != 0] & ~np.uint32(T.T_SHIFTED)) == T.T_AGREES).all()


@pytest.mark.parametrize("pair", list(itertools.product((0, 1), (0, 1))))
def test_a_second_call_on_the_result_agrees_and_changes_nothing(eng, pair):
    la = TC.launch(40, 33, 12, seed=4)
    cfg = TC.cfg(12, *pair)
    first = _call(eng, la, cfg, True)
    second = _call(eng, la, cfg, True, arrays=first[2:])
    assert all(second[k].tobytes() == first[k].tobytes() for k in (2, 3, 4))
    was_aided = (first[0]["flags"] & T.T_AIDED) != 0
    assert was_aided.any() and ((second[0]["flags"][was_aided] & ~np.uint32(T.T_SHIFTED)) == T.T_AGREES).all() and not second[1]["n_aided"].any()
    assert (second[1]["valid_after_mask"] == first[1]["valid_after_mask"]).all()
    la.sync, la.states, la.obs = first[2:]
    _same(second, TC.run(la, cfg), "second")


def test_receivers_permuted_give_the_same_bytes_permuted(eng):
    la, lb = TC.launch(13, 12, 5), TC.launch(13, 12, 5)
    perm = np.random.default_rng(5).permutation(la.n_rx)
    slots = (perm[:, None] * la.ch + np.arange(la.ch)[None, :]).reshape(-1)
    lb.pred_rx, lb.pred = np.ascontiguousarray(la.pred_rx[perm]), np.ascontiguousarray(la.pred[perm])
    lb.sync, lb.states, lb.obs = (np.ascontiguousarray(v[slots]) for v in (la.sync, la.states, la.obs))
    cfg = TC.cfg(5, 1, 1)
    a, b = _call(eng, la, cfg, True), _call(eng, lb, cfg, True)
    assert a[0][slots].tobytes() == b[0].tobytes() and a[1][perm].tobytes() == b[1].tobytes()
    assert all(a[k][slots].tobytes() == b[k].tobytes() for k in (2, 3, 4))


def test_refusals_come_with_their_text_and_write_nothing(eng):
    la = TC.launch(3)
    nan, inf = float("nan"), float("inf")
    good = dict(null=None, sigma=30.0, resid=8.0, ch=la.ch, age=40, resolve=1, rearm=1, reserved=0, n_rx=la.n_rx, n_prn=la.n_prn, prns=[int(v) for v in la.prns], off={},
                alias=None)
    by_message = {
        b"null argument": [dict(null=w) for w in ("cfg", "prns", "pred_rx", "pred", "sync", "states", "tow", "tow_rx")] + [dict(null="tow", ch=0)],
        b"max_sigma_m must be finite and above 0": [dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf, resid=0.0)],
        b"max_resid_samples must be finite, above 0 and at most 4092": [dict(resid=0.0), dict(resid=-8.0), dict(resid=nan), dict(resid=inf), dict(resid=4092.5, ch=0)],
        b"ch_per_rx must be 1..64": [dict(ch=0), dict(ch=65), dict(ch=-1, age=-1)],
        b"max_age_blocks must be 0..4096": [dict(age=-1), dict(age=4097, resolve=2)],
        b"resolve and rearm must be 0 or 1": [dict(resolve=2), dict(resolve=-1), dict(rearm=2), dict(rearm=-1, reserved=1)],
        b"reserved must be 0": [dict(reserved=1), dict(reserved=-1, n_rx=0)],
        b"n_rx must be 1..1048576": [dict(n_rx=0), dict(n_rx=(1 << 20) + 1, n_prn=0)],
        b"n_prn must be 1..64": [dict(n_prn=0), dict(n_prn=65, prns=list(range(1, 66)))],
        b"PRN outside 1..210": [dict(prns=[0] + good["prns"][1:]), dict(prns=good["prns"][:-1] + [211])],
        b"a PRN is listed twice": [dict(prns=good["prns"][:-1] + good["prns"][:1]), dict(prns=[7] * la.n_prn, off=dict(pred=8))],
        b"d_pred_rx, d_pred, d_obs_state and d_obs must be 16-byte aligned": [dict(off=dict(pred_rx=8)), dict(off=dict(pred=8)), dict(off=dict(states=8)),
                                                                              dict(off=dict(obs=8, sync=4))],
        b"d_sync_state must be 8-byte aligned": [dict(off=dict(sync=4)), dict(off=dict(sync=4, tow=8))],
        b"d_tow or d_tow_rx overlaps another array": [dict(alias=("tow", w)) for w in ("pred_rx", "pred", "sync", "states", "obs")] +
                                                     [dict(alias=("tow_rx", w)) for w in ("pred_rx", "pred", "sync", "states", "obs", "tow")],
    }
    dev_only = {b"d_tow and d_tow_rx must be 16-byte aligned": [dict(off=dict(tow=8)), dict(off=dict(tow_rx=8))]}
    n_ch = la.n_rx * la.ch
    with G.Pool() as pool:
        ins = {k: pool.add(G.Guarded(eng, a.nbytes, G.STATE_FILL, a)) for k, a in (("pred_rx", la.pred_rx), ("pred", la.pred), ("sync", la.sync), ("states", la.states),
                                                                                   ("obs", la.obs))}
        outs = {dev: dict(tow=pool.add(G.Guarded(eng if dev else None, n_ch * 32)), tow_rx=pool.add(G.Guarded(eng if dev else None, la.n_rx * 64))) for dev in (True, False)}
        fns = {True: eng.lib.gpsx_wtow_dev, False: eng.lib.gpsx_wtow}

        def call(a, dev):
            cfg = T.make_cfg(a["ch"], a["sigma"], a["resid"], a["age"], a["resolve"], a["rearm"])
            cfg["reserved"] = a["reserved"]
            prns = np.array(a["prns"], np.uint8)
            at = dict(ins, **outs[dev])

            def ptr(name):
                if a["null"] == name:
                    return None
                if a["alias"] and a["alias"][0] == name:      # the output's last byte on the other array's first
                    size = n_ch * 32 if name == "tow" else la.n_rx * 64
                    return C.c_void_p(at[a["alias"][1]].ptr.value - size + 16)
                return C.c_void_p(at[name].ptr.value + a["off"].get(name, 0))
            return fns[dev](eng.h, None if a["null"] == "cfg" else cfg.ctypes.data, a["n_rx"], a["n_prn"], None if a["null"] == "prns" else prns.ctypes.data,
                            ptr("pred_rx"), ptr("pred"), ptr("sync"), ptr("states"), ptr("obs"), ptr("tow"), ptr("tow_rx"))
        bufs = [*ins.values(), *outs[True].values(), *outs[False].values()]
        G.refusals(eng, by_message, good, call, bufs)
        for message, changes in dev_only.items():
            for change in changes:
                for b in bufs:
                    b.refill()
                assert call({**good, **change}, True) == EINVAL and eng.lib.gpsx_last_error(eng.h) == message, (change, eng.lib.gpsx_last_error(eng.h))
                eng.synchronize()
                assert all(b.untouched() for b in bufs), change
        for change in (dict(age=4096), dict(age=0, resid=4092.0), dict(resolve=0, rearm=0, null="obs"), dict(sigma=1e300)):
            for dev in (False, True):
                assert call({**good, **change}, dev) == 0, (change, eng.lib.gpsx_last_error(eng.h))
                assert eng.lib.gpsx_synchronize(eng.h) == 0


def test_behind_the_device_stages_both_call_orders(eng):
    """weighted_pvt_cases' stream through weighted_gpu.Chain with gpsx_wbank_dev, gpsx_wfix_dev, gpsx_wvel_dev and gpsx_wkf_dev after every
    launch, as tests/test_gpu_weighted_pred.py's stream test is built.  At block 24 576 the states are copied to a second set of buffers
    whose four observable states are cleared, as a hand-over clears them; both sets run the last 424 blocks.  The cleared set ends with
    PHASE | EDGE and no VALID slot.  After gpsx_wkf_dev: gpsx_wpred_dev with lead_blocks 0 on the filter's state of block 25 000 and
    gpsx_wtow_dev make all four AIDED, with the undisturbed set's tx_ms, the device's bytes equal to the restatement's on the device's own
    records, and |rho| within 1.5 x weighted_tow_cases.MEASURED.  Before gpsx_wkf_dev: gpsx_wpred_dev with lead_blocks 424 on the filter's
    state of block 24 576, gpsx_wtow_dev with d_obs, then gpsx_wkf_dev on the cleared set's observables: four pseudorange rows, where
    without the stage it has none.  Cost: the stream's synthesis (about 25 s of CPU, cached per process) and its upload, plus a few
    seconds of GPU."""
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
    tcfg = T.make_cfg(n_ch, **TC.STREAM)
    bank0 = P.empty_bank(1, len(prns))
    a = G.Chain(eng, S.sync_cfg_dev(S.MOVING), dict(S.fresh_states(), sync=S.handover()), max(S.LAUNCHES), S.MAX_BAD_WORDS, S.EDGE_GUARD)
    b = None
    bufs = dict(bank=G.Guarded(eng, bank0.nbytes, G.STATE_FILL, bank0), out=G.Guarded(eng, n_ch * 256), rep=G.Guarded(eng, 32), fix=G.Guarded(eng, F.FIX_DTYPE.itemsize),
                vel=G.Guarded(eng, V.VEL_DTYPE.itemsize), kf=G.Guarded(eng, R.KF_DTYPE.itemsize), state=G.Guarded(eng, 384, G.STATE_FILL, np.zeros(1, R.STATE_DTYPE)),
                state2=G.Guarded(eng, 384, G.STATE_FILL, np.zeros(1, R.STATE_DTYPE)), rx=G.Guarded(eng, 64), pred=G.Guarded(eng, len(prns) * 64),
                tow=G.Guarded(eng, n_ch * 32), tow_rx=G.Guarded(eng, 64))

    def wkf(chain, state, n):
        eng._chk(lib.gpsx_wkf_dev(eng.h, kcfg.ctypes.data, chain.buf["o"].ptr, bufs["out"].ptr, None, bufs["fix"].ptr, bufs["vel"].ptr, 1, n, bufs[state].ptr,
                                  bufs["kf"].ptr), "wkf")

    def aid(state, lead):
        """gpsx_wpred_dev (predict only) on the filter state in bufs[state], then gpsx_wtow_dev on the cleared set -> (rx, pred, tow, tow_rx)"""
        for name in ("rx", "pred", "tow", "tow_rx"):
            bufs[name].refill()
        pcfg = PC.stream_cfg(0)
        pcfg["lead_blocks"] = lead
        eng._chk(lib.gpsx_wpred_dev(eng.h, pcfg.ctypes.data, 1, len(prns), prns.ctypes.data, bufs[state].ptr, bufs["bank"].ptr, b.buf["sync"].ptr, None, None, None, None,
                                    bufs["rx"].ptr, bufs["pred"].ptr), "gpsx_wpred_dev")
        eng._chk(lib.gpsx_wtow_dev(eng.h, tcfg.ctypes.data, 1, len(prns), prns.ctypes.data, bufs["rx"].ptr, bufs["pred"].ptr, b.buf["sync"].ptr, b.buf["obs"].ptr,
                                   b.buf["o"].ptr, bufs["tow"].ptr, bufs["tow_rx"].ptr), "gpsx_wtow_dev")
        assert lib.gpsx_last_kernel(eng.h) == b"k_wtow"
        eng.synchronize()
        return (bufs["rx"].get(P.PRED_RX_DTYPE, (1,)), bufs["pred"].get(P.PRED_DTYPE, (1, len(prns))), bufs["tow"].get(T.TOW_DTYPE, (n_ch,)),
                bufs["tow_rx"].get(T.TOW_RX_DTYPE, (1,)))
    try:
        at = 0
        for k, n in enumerate(S.LAUNCHES):
            last = k == len(S.LAUNCHES) - 1
            if last:
                state_24576 = bufs["state"].get(R.STATE_DTYPE, (1,))
                st_b = {name: a.read(name) for name in ("sync", "nav", "obs", "eph")}
                st_b["obs"] = np.zeros(n_ch, O.STATE_DTYPE)
                b = G.Chain(eng, S.sync_cfg_dev(S.MOVING), st_b, max(S.LAUNCHES), S.MAX_BAD_WORDS, S.EDGE_GUARD)
                b.sync(d_if + at * 4092, n)
                b.words()
                b.obs()
            a.sync(d_if + at * 4092, n)
            a.words()
            a.obs()
            a.eph()
            eng._chk(lib.gpsx_wbank_dev(eng.h, bcfg.ctypes.data, 1, len(prns), prns.ctypes.data, a.buf["sync"].ptr, a.buf["e"].ptr, bufs["bank"].ptr, bufs["out"].ptr,
                                        bufs["rep"].ptr), "gpsx_wbank_dev")
            eng._chk(lib.gpsx_wfix_dev(eng.h, fcfg.ctypes.data, a.buf["o"].ptr, bufs["out"].ptr, None, bufs["fix"].ptr if at else None, 1, bufs["fix"].ptr, None), "wfix")
            eng._chk(lib.gpsx_wvel_dev(eng.h, vcfg.ctypes.data, a.buf["o"].ptr, bufs["out"].ptr, None, bufs["fix"].ptr, 1, bufs["vel"].ptr), "wvel")
            wkf(a, "state", n)
            eng.synchronize()
            at += n
        assert at == 25000 and int(bufs["kf"].get(R.KF_DTYPE, 1)["flags"][0]) & R.F_UPDATED
        und, fresh_st, fresh_o = a.read("o"), b.read("obs"), b.read("o")
        need = O.F_PHASE | O.F_EDGE
        assert (und["flags"] & O.F_VALID).all() and ((fresh_o["flags"] & need) == need).all() and not (fresh_o["flags"] & (O.F_TOW | O.F_VALID)).any()
        assert (fresh_st["blocks_seen"] == n).all() and b.read("sync").tobytes() == a.read("sync").tobytes()
        # -- after gpsx_wkf_dev, lead_blocks 0: the aided slot counts from the next launch on
        rx, pred, tow, tow_rx = aid("state", 0)
        sync_now, w_st, w_o = b.read("sync"), fresh_st.copy(), fresh_o.copy()
        w_tow, w_tow_rx = T.run(tcfg, prns, rx, pred, sync_now.copy(), w_st, w_o)
        print("records", tow, "undisturbed tx_ms", und["tx_ms"], "|rho| at most", float(np.abs(tow["resid"]).max()))
        assert tow.tobytes() == w_tow.tobytes() and tow_rx.tobytes() == w_tow_rx.tobytes() and b.read("obs").tobytes() == w_st.tobytes() and b.read("o").tobytes() == w_o.tobytes()
        assert int(rx["t_ms"][0]) == int(round(S.TOW0 * 1000.0)) + 25000 and (tow["flags"] == T.T_AIDED).all() and int(tow_rx["valid_after_mask"][0]) == 15
        aided_o = b.read("o")
        assert aided_o["tx_ms"].tolist() == und["tx_ms"].tolist() and (aided_o["flags"] & O.F_VALID).all() and not (aided_o["flags"] & O.F_AMBIGUOUS).any()
        assert b.read("sync").tobytes() == sync_now.tobytes()
        assert float(np.abs(tow["resid"]).max()) <= 1.5 * TC.MEASURED["resid_samples"]
        # -- before gpsx_wkf_dev, lead_blocks = n_blocks on the filter state of the launch before: the aided slot counts in this launch
        rows = {}
        for with_stage in (False, True):
            b.buf["obs"].put(fresh_st)
            b.buf["o"].put(fresh_o)
            bufs["state2"].put(state_24576)
            if with_stage:
                rx, pred, tow, tow_rx = aid("state2", n)
                assert int(rx["t_ms"][0]) == int(round(S.TOW0 * 1000.0)) + 25000 and (tow["flags"] == T.T_AIDED).all()
                assert b.read("o")["tx_ms"].tolist() == und["tx_ms"].tolist()
            bufs["kf"].refill()
            wkf(b, "state2", n)
            eng.synchronize()
            rec = bufs["kf"].get(R.KF_DTYPE, 1)[0]
            rows[with_stage] = (int(rec["n_pr"]), int(rec["pr_mask"]))
        print("pseudorange rows of the launch: without the stage", rows[False], "with it", rows[True])
        assert rows[False] == (0, 0) and rows[True] == (4, 15)
    finally:
        for buf in bufs.values():
            buf.free()
        a.free()
        if b is not None:
            b.free()
        eng.free(d_if)
