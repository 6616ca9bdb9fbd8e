"""Build recipe for libgpsx.so (hipcc, gfx950, in-tree).  `python -m stm32f4_sdr_gps_amd.build` or build.build()."""
from __future__ import annotations

import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(PKG, "lib", "libgpsx.so")
LAB_LIB = os.path.join(PKG, "lib", "libgpsx_lab.so")
LLVM_BIN = "/opt/rocm/lib/llvm/bin"
# the matrix-core grid's objects: the single-block / walk / store / split forms, the byte-phase form, the weighted kernels
MX_OBJECTS = ("k_acq_mx.o", "k_acq_mx_byte.o", "k_acq_mxw.o")


def build(verbose: bool = False, jobs: int = 4) -> str:
    """Compile every HIP source for gfx950 and link lib/libgpsx.so.  Cross-compiles without a GPU."""
    env = dict(os.environ)
    env.setdefault("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = ["make", "-C", os.path.join(PKG, "csrc"), f"-j{jobs}"]
    res = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        sys.stderr.write(res.stdout)
    if res.returncode != 0 or not os.path.exists(LIB) or not os.path.exists(LAB_LIB):
        raise RuntimeError("building libgpsx.so failed")
    check_no_scratch()
    return LIB


def unbundle_gfx950(obj: str, img: str) -> None:
    """Write the gfx950 code object inside the host object `obj` (its .hip_fatbin offload bundle) to `img`."""
    raw = open(obj, "rb").read()
    at = raw.find(b"__CLANG_OFFLOAD_BUNDLE__")
    if at < 0:
        raise RuntimeError(f"{obj}: no offload bundle inside")
    fat = img + ".fatbin"
    with open(fat, "wb") as f:
        f.write(raw[at:])
    subprocess.check_call([os.path.join(LLVM_BIN, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={img}"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    os.remove(fat)


def kernel_resources(obj: str | None = None) -> dict:
    """{kernel symbol: {"vgprs", "sgprs", "scratch_bytes", "lds_bytes"}} of the device code in the object file `obj` (default:
    build/k_acq_mx.o, the first of MX_OBJECTS), read from the code object's metadata notes (llvm-readelf --notes on the unbundled
    gfx950 image)."""
    import re
    import tempfile
    obj = obj or os.path.join(PKG, "build", MX_OBJECTS[0])
    with tempfile.TemporaryDirectory() as tmp:
        img = os.path.join(tmp, "dev.co")
        unbundle_gfx950(obj, img)
        notes = subprocess.check_output([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", img], text=True)
    out = {}
    for blk in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))   # noqa: E731
        out[name.group(1)] = {"vgprs": get("vgpr_count"), "sgprs": get("sgpr_count"), "scratch_bytes": get("private_segment_fixed_size"),
                              "lds_bytes": get("group_segment_fixed_size")}
    return out


def check_no_scratch() -> dict:
    """The matrix-core grid kernels live one register from the spill cliff (k_acq_mx<3>: 255 VGPRs): a build whose k_acq_mx
    instance spills to scratch memory is refused here, not discovered as a slow kernel on the GPU box."""
    res = {}
    for name in MX_OBJECTS:   # (no kernel is in two of them)
        res.update(kernel_resources(os.path.join(PKG, "build", name)))
    mx = {k: v for k, v in res.items() if "k_acq_mx" in k}
    # ... the weighted grid's multi-block matrix-core kernel beside them (its own name: the counts above are k_acq_mx's)
    wmx = {k: v for k, v in res.items() if "k_acq_wmx" in k}
    if len(wmx) != 1:
        raise RuntimeError(f"expected k_acq_wmx_ms in build/k_acq_mxw.o, found {sorted(wmx)}")
    if not mx:
        raise RuntimeError(f"no k_acq_mx kernels found in the code object metadata of {MX_OBJECTS}")
    # ... and the device tracking loops, whose occupancy (three waves per SIMD: 168 VGPRs) is asked for by __launch_bounds__
    loops = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_track_loop.o")).items() if "k_track_loop" in k}
    if len(loops) != 4:
        raise RuntimeError(f"expected four k_track_loop instances, found {sorted(loops)}")
    # ... and the weighted grid's vector-ALU kernels (k_acq_weighted_ms keeps 32 running sums per thread in registers)
    wv = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_acq_weighted.o")).items() if "k_acq_weighted" in k}
    if len(wv) != 2:
        raise RuntimeError(f"expected k_acq_weighted and k_acq_weighted_ms, found {sorted(wv)}")
    # ... and the coherent weighted grid's two kernels (no scratch by design: the pre-summed blocks live in LDS)
    coh = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_acq_coh.o")).items() if "k_acq_coh" in k}
    if len(coh) != 2 or not all(any(k in name for name in coh) for k in ("k_acq_coh_mx", "k_acq_coh_vec")):
        raise RuntimeError(f"expected k_acq_coh_mx and k_acq_coh_vec in build/k_acq_coh.o, found {sorted(coh)}")
    # ... and the hybrid (coherent windows summed non-coherently) grid's two, in an object and under names of their own
    hyb = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_acq_hyb.o")).items() if "k_acq_hyb" in k}
    if len(hyb) != 2 or not all(any(k in name for name in hyb) for k in ("k_acq_hyb_mx", "k_acq_hyb_vec")):
        raise RuntimeError(f"expected k_acq_hyb_mx and k_acq_hyb_vec in build/k_acq_hyb.o, found {sorted(hyb)}")
    # ... and the weighted E/P/L correlators (twelve counters and sixteen plane words per lane: no spill by a wide margin)
    trw = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_track_weighted.o")).items() if "k_track_epl_weighted" in k}
    if len(trw) != 1:
        raise RuntimeError(f"expected k_track_epl_weighted in build/k_track_weighted.o, found {sorted(trw)}")
    # ... and the closed loop behind them (k_track_wloop: the same correlator body, ten state words and the loop's floats on top)
    wloop = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_track_loop_weighted.o")).items() if "k_track_wloop" in k}
    if len(wloop) != 1:
        raise RuntimeError(f"expected k_track_wloop in build/k_track_loop_weighted.o, found {sorted(wloop)}")
    # ... and the loop with the bit synchroniser (k_track_wsync: the open window and the synchroniser's words on top of that; the
    #     update, state image and lane places of both loops are one header, gpsx_track_wloop_parts.hpp)
    wsync = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_track_loop_weighted_sync.o")).items() if "k_track_wsync" in k}
    if len(wsync) != 1:
        raise RuntimeError(f"expected k_track_wsync in build/k_track_loop_weighted_sync.o, found {sorted(wsync)}")
    # ... and the carrier-aided instance of each loop (k_track_waid_loop, k_track_waid_sync: the same kernel texts with window_update's
    #     aiding clause, in the same objects; names of their own, so that the two counts above stay counts of the unaided kernels).
    #     The same occupancy is asked of them: four waves per SIMD, 128 VGPRs
    waid = {}
    for obj, name in (("k_track_loop_weighted.o", "k_track_waid_loop"), ("k_track_loop_weighted_sync.o", "k_track_waid_sync")):
        hits = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", obj)).items() if name in k}
        if len(hits) != 1:
            raise RuntimeError(f"expected {name} in build/{obj}, found {sorted(hits)}")
        waid.update(hits)
    wide = {k: v for k, v in waid.items() if v["vgprs"] > 128}
    if wide:
        raise RuntimeError(f"carrier-aided loop kernels above 128 VGPRs (four waves per SIMD): {wide}")
    # ... and the sync loop for many receivers per launch (check_wmulti below: refused here like the others; not in the table this
    #     returns, whose keys callers search for the single-stream kernels' names, which k_track_wsync_multi's contains)
    check_wmulti()
    # ... and the position fixes at the chain's end (check_wfix below: FP64 with a dozen libm calls per row, refused here if it spills)
    check_wfix()
    # ... and the fixes with millisecond repair and fault exclusion (check_wfde below: k_wfix's solver inside a loop over rounds)
    check_wfde()
    # ... and the velocity fixes behind either (check_wvel below: one linear solve per receiver, no scratch and no LDS)
    check_wvel()
    # ... and the navigation filter behind them (check_wkf below: two 8 x 8 factorisations per receiver in registers, no scratch, no LDS)
    check_wkf()
    # ... and, between the grids and the loops, the acquisition decisions (check_wacq below: a wave per receiver, no scratch, no LDS)
    check_wacq()
    # ... and, behind the ephemeris stage, the ephemeris bank (check_wbank below: the same terms)
    check_wbank()
    # ... and, behind the filter, the prediction and hot hand-over (check_wpred below: FP64, a wave per receiver, the same terms)
    check_wpred()
    # ... and, behind the observables and the prediction, the time-of-week aiding (check_wtow below: the same terms)
    check_wtow()
    # ... and, beside the ephemeris stage, the almanac, ionosphere and UTC (check_walm below: the same terms)
    check_walm()
    # ... and, between the prediction and the acquisition decisions, the grid in a window (check_wwin below: no scratch, its LDS as planned)
    check_wwin()
    # ... and, behind any weighted grid, the snapshot fixes (check_wsnap below: FP64, a wave per receiver, no scratch, no LDS)
    check_wsnap()
    # ... and the word layer behind it (k_wnav_words: two register sets of eight slots' bit words, the frame state)
    wnav = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_wnav_words.o")).items() if "k_wnav_words" in k}
    if len(wnav) != 1:
        raise RuntimeError(f"expected k_wnav_words in build/k_wnav_words.o, found {sorted(wnav)}")
    # ... and the observables behind both (k_wobs: two register sets of eight slots' four words, eight word records, the state)
    wobs = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_wobs.o")).items() if "k_wobs" in k}
    if len(wobs) != 1:
        raise RuntimeError(f"expected k_wobs in build/k_wobs.o, found {sorted(wobs)}")
    # ... and the ephemerides behind the words (k_weph: eight word records, the state's 48 words and the record's 64 in registers,
    #     cur[] / sf[][] reached through select chains, never through an index; 17 KiB of LDS stage the records' stores)
    weph = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_weph.o")).items() if "k_weph" in k}
    if len(weph) != 1:
        raise RuntimeError(f"expected k_weph in build/k_weph.o, found {sorted(weph)}")
    # ... and the lock monitor on the records (k_wlock: two register sets of four slots' eight words, five int64 sums, the state)
    wlock = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_wlock.o")).items() if "k_wlock" in k}
    if len(wlock) != 1:
        raise RuntimeError(f"expected k_wlock in build/k_wlock.o, found {sorted(wlock)}")
    every = {**mx, **wmx, **loops, **wv, **coh, **hyb, **trw, **wloop, **wsync, **waid, **wnav, **wobs, **weph, **wlock}
    bad = {k: v for k, v in every.items() if v["scratch_bytes"] != 0}
    if bad:
        raise RuntimeError(f"kernels with scratch memory (register spills): {bad}")
    return every


def check_wmulti() -> dict:
    """k_track_wsync_multi (the aided sync kernel's text a third time, a workgroup per receiver; an object of its own): exactly one
    instance, no scratch, and k_track_waid_sync's occupancy -- four waves per SIMD, 128 VGPRs at most.  -> {symbol: resources}"""
    wmulti = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", "k_track_loop_weighted_sync_multi.o")).items() if "k_track_wsync_multi" in k}
    if len(wmulti) != 1:
        raise RuntimeError(f"expected k_track_wsync_multi in build/k_track_loop_weighted_sync_multi.o, found {sorted(wmulti)}")
    bad = {k: v for k, v in wmulti.items() if v["vgprs"] > 128 or v["scratch_bytes"] != 0}
    if bad:
        raise RuntimeError(f"multi-receiver sync loop kernel above 128 VGPRs (four waves per SIMD) or with scratch memory: {bad}")
    return wmulti


def check_wsolver(obj: str, kernel: str, no_lds: bool) -> dict:
    """One solver kernel at the weighted chain's end (a slot per lane, a receiver's system in registers, the shared parts from
    csrc/gpsx_wsolve_parts.hpp; an object of its own): exactly one instance in build/`obj`, no scratch and, if `no_lds`, no LDS.
    -> {symbol: resources}"""
    found = {k: v for k, v in kernel_resources(os.path.join(PKG, "build", obj)).items() if kernel in k}
    if len(found) != 1:
        raise RuntimeError(f"expected {kernel} in build/{obj}, found {sorted(found)}")
    bad = {k: v for k, v in found.items() if v["scratch_bytes"] != 0 or (no_lds and v["lds_bytes"] != 0)}
    if bad:
        raise RuntimeError(f"{kernel} with scratch memory (register spills){' or LDS' if no_lds else ''}: {bad}")
    return found


def check_wfix() -> dict:
    """k_wfix, every receiver's position fix"""
    return check_wsolver("k_wfix.o", "k_wfix", False)


def check_wfde() -> dict:
    """k_wfde, the fixes with millisecond repair and fault exclusion"""
    return check_wsolver("k_wfde.o", "k_wfde", False)


def check_wvel() -> dict:
    """k_wvel, every receiver's velocity and clock drift: no LDS either"""
    return check_wsolver("k_wvel.o", "k_wvel", True)


def check_wkf() -> dict:
    """k_wkf, every receiver's navigation filter: no LDS either"""
    return check_wsolver("k_wkf.o", "k_wkf", True)


def check_wacq() -> dict:
    """k_wacq, acquisition decisions and slot hand-over (not a solver, but the same terms: an object of its own, exactly one instance,
    no scratch and no LDS)"""
    return check_wsolver("k_wacq.o", "k_wacq", True)


def check_wbank() -> dict:
    """k_wbank, the ephemeris bank (a mover of records, in the solvers' terms: an object of its own, exactly one instance, no scratch
    and no LDS)"""
    return check_wsolver("k_wbank.o", "k_wbank", True)


def check_wpred() -> dict:
    """k_wpred, prediction and hot hand-over (the solvers' shared parts on k_wacq's geometry: an object of its own, exactly one
    instance, no scratch and no LDS)"""
    return check_wsolver("k_wpred.o", "k_wpred", True)


def check_wtow() -> dict:
    """k_wtow, time-of-week aiding of the observables (a mover of a few words per slot on k_wacq's geometry: an object of its own,
    exactly one instance, no scratch and no LDS)"""
    return check_wsolver("k_wtow.o", "k_wtow", True)


def check_walm() -> dict:
    """k_walm, almanac, ionosphere and UTC from subframes 4 and 5 (k_weph's assembly on k_wbank's geometry: an object of its own,
    exactly one instance, no scratch and no LDS)"""
    return check_wsolver("k_walm.o", "k_walm", True)


def check_wsnap() -> dict:
    """k_wsnap, snapshot fixes from a weighted grid's records, a bank and a prior (the solvers' shared parts on k_wacq's geometry, a
    5 x 5 system in every lane's registers: an object of its own, exactly one instance, no scratch and no LDS)"""
    return check_wsolver("k_wsnap.o", "k_wsnap", True)


# k_acq_win's LDS: the planes (2 x 16 x 1024 int8), the two int16 rows (2 x 1028 dwords), the chip pairs (512 dwords), E (4096 dwords),
# the four waves' keys, far sums (8 bytes each) and far counts
WWIN_LDS_BYTES = 2 * 16 * 1024 + 2 * 1028 * 4 + 512 * 4 + 4096 * 4 + 4 * (8 + 8 + 4)


def check_wwin() -> dict:
    """k_acq_win, the weighted grid in a window around each prediction (the coherent grids' parts on one PRN and a slice of the phases:
    an object of its own, exactly one instance, no scratch, and the LDS it was planned with -- two workgroups per compute unit)"""
    found = check_wsolver("k_acq_win.o", "k_acq_win", False)
    bad = {k: v for k, v in found.items() if v["lds_bytes"] != WWIN_LDS_BYTES}
    if bad:
        raise RuntimeError(f"k_acq_win's LDS is not the planned {WWIN_LDS_BYTES} bytes: {bad}")
    return found


if __name__ == "__main__":
    print(build(verbose=True))
