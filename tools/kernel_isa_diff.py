#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, instruction by instruction.

    python tools/kernel_isa_diff.py OLD.o [OLD2.o ...] -- NEW.o [NEW2.o ...]

e.g. the parent commit's build/k_acq_mx.o against this tree's build/k_acq_mx.o build/k_acq_mx_byte.o build/k_acq_mxw.o: the proof
a refactor of kernels that sit at the register limit owes (a timing cannot tell 0 % from 1 %).  Each object's gfx950 image is
unbundled (build.unbundle_gfx950) and disassembled with llvm-objdump -d; the listing is split by kernel symbol and normalised:
  * addresses and raw instruction bytes are dropped;
  * the 32-bit literal of the add / add-with-carry pair behind an s_getpc_b64 is masked: a pc-relative address of a constant,
    which moves with the kernel's position in the image;
  * the padding behind a kernel's last instruction (the trailing run of s_nop / s_code_end) is dropped -- and only that: the
    compiler lays cold blocks behind the last s_endpgm.
Per kernel: instruction counts, the number of differing lines and the first of them, and VGPRs / SGPRs / LDS / scratch of both
sides (build.kernel_resources).  Exit status 1 if a kernel that both sides have differs, 0 otherwise.  Needs no GPU.
"""
from __future__ import annotations

import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from stm32f4_sdr_gps_amd import build  # noqa: E402

SHOWN = int(os.environ.get("ISA_DIFF_SHOWN", "6"))   # differing lines printed per kernel


def kernels(objs: list[str]) -> tuple[dict, dict]:
    """({kernel symbol: [normalised instruction lines]}, {kernel symbol: resources}) of the objects' gfx950 images"""
    code, res = {}, {}
    for obj in objs:
        meta = build.kernel_resources(obj)
        res.update(meta)
        with tempfile.TemporaryDirectory() as tmp:
            img = os.path.join(tmp, "dev.co")
            build.unbundle_gfx950(obj, img)
            listing = subprocess.check_output([os.path.join(build.LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                               img], text=True)
        name = None
        for line in listing.splitlines():
            head = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line)
            if head:
                name = head.group(1) if head.group(1) in meta else None   # (kernels only: not the labels inside them)
                if name:
                    code[name] = []
                continue
            text = re.sub(r"\s*//.*$", "", line).strip()   # (the trailing comment: address and encoding)
            if name and text:
                code[name].append(re.sub(r"\s+", " ", text))
    for name, lines in code.items():
        while lines and re.match(r"(s_nop|s_code_end)\b|\.\.\.$", lines[-1]):   # (cold blocks behind the last s_endpgm are code)
            del lines[-1]
        pc_at = -9
        for i, text in enumerate(lines):
            if text.startswith("s_getpc_b64"):
                pc_at = i
            elif i - pc_at <= 2 and re.match(r"s_addc?_u32 ", text):
                lines[i] = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pc-relative>", text)
    return code, res


def short_name(symbol: str) -> str:
    """gpsx::<kernel>, with an integer template argument if it has one, of a mangled kernel symbol"""
    m = re.match(r"_ZN4gpsx(\d+)", symbol)
    if not m:
        return symbol
    name, rest = symbol[m.end():][:int(m.group(1))], symbol[m.end() + int(m.group(1)):]
    arg = re.match(r"ILi(\d+)E", rest)
    return f"gpsx::{name}<{arg.group(1)}>" if arg else f"gpsx::{name}"


def main(argv: list[str]) -> int:
    if "--" not in argv or argv[0] == "--" or argv[-1] == "--":
        sys.stderr.write(__doc__)
        return 2
    at = argv.index("--")
    (old, old_res), (new, new_res) = kernels(argv[:at]), kernels(argv[at + 1:])
    differing = 0
    for name in sorted(set(old) | set(new)):
        demangled = short_name(name)
        if name not in old or name not in new:
            print(f"{demangled}: only in the {'old' if name in old else 'new'} build")
            continue
        a, b = old[name], new[name]
        changed = [line for line in difflib.unified_diff(a, b, lineterm="", n=0) if line[0] in "+-" and line[:3] not in ("+++", "---")]
        fmt = lambda r: f"{r['vgprs']} VGPRs, {r['sgprs']} SGPRs, {r['lds_bytes']} B LDS, {r['scratch_bytes']} B scratch"   # noqa: E731
        print(f"{demangled}: {len(a)} / {len(b)} instructions, {len(changed)} differing lines"
              f"{'' if changed else ' -- identical'}\n    old: {fmt(old_res[name])}\n    new: {fmt(new_res[name])}")
        for line in changed[:SHOWN]:
            print(f"      {line}")
        differing += bool(changed) or old_res[name] != new_res[name]
    print(f"{differing} kernel(s) differ")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
