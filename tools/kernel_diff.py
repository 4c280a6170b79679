#!/usr/bin/env python3
"""Compare the device code of two builds of csrc/, kernel by kernel (CPU only; it compares, it looks for no instruction).

Inputs are two directories of device assembly, one .s per source file, made with the Makefile's flags plus
--cuda-device-only -S, from the commit before a change and from the commit with it:

    cd recbole-cdr_amd/csrc && mkdir -p /tmp/asm_a && for f in *.hip; do hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC \
        -munsafe-fp-atomics -Wno-unused-result --cuda-device-only -S $f -o /tmp/asm_a/${f%.hip}.s; done     # at the parent
    (the same at the new commit into /tmp/asm_b), then:  python tools/kernel_diff.py /tmp/asm_a /tmp/asm_b

Kernels are paired by (file, symbol).  Per kernel: is the text identical (comments dropped, block labels numbered in order of
appearance), are the resource fields identical, is the opcode histogram (mnemonics only) identical.  --ignore a,b leaves the
named mnemonics out of the histogram comparison; -v lists every kernel, not only the ones that differ.  Exit status 1 if any
kernel is missing on one side or differs in resources or histogram.
"""
import argparse
import collections
import pathlib
import re
import sys

FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    """{symbol: (text lines, {field: value}, Counter of mnemonics)} of one .s file."""
    lines = path.read_text().splitlines()
    res, sym = {}, None
    for ln in lines:                                            # the .amdhsa_kernel blocks name the kernels and their resources
        t = ln.split()
        if t[:1] == [".amdhsa_kernel"]:
            sym = t[1]; res[sym] = {}
        elif t[:1] == [".end_amdhsa_kernel"]:
            sym = None
        elif sym and t and t[0].startswith(".amdhsa_") and t[0][8:] in FIELDS:
            res[sym][t[0][8:]] = t[1]
    out, sym, body = {}, None, []
    for ln in lines:
        ln = ln.split(";")[0].strip()
        if not ln:
            continue
        if sym is None:
            if ln.endswith(":") and ln[:-1] in res:
                sym, body = ln[:-1], []
        elif ln.startswith(".Lfunc_end"):
            ops = collections.Counter(x.split()[0] for x in body if not x.startswith(".") and not x.endswith(":"))
            lab = {}                                            # block labels numbered in order of appearance
            body = [re.sub(r"\.L(?:BB|tmp|JTI)\d+_\d+", lambda m: lab.setdefault(m.group(0), f".L{len(lab)}"), x) for x in body]
            out[sym] = (body, res[sym], ops); sym = None
        else:
            body.append(ln)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dir_a"); ap.add_argument("dir_b")
    ap.add_argument("--ignore", default="", help="comma-separated mnemonics left out of the histogram comparison")
    ap.add_argument("-v", action="store_true")
    a = ap.parse_args()
    ign = set(filter(None, a.ignore.split(",")))
    n = same = reorder = bad = 0
    names = sorted({p.name for d in (a.dir_a, a.dir_b) for p in pathlib.Path(d).glob("*.s")})
    for name in names:
        pa, pb = pathlib.Path(a.dir_a, name), pathlib.Path(a.dir_b, name)
        ka, kb = (kernels(p) if p.exists() else {} for p in (pa, pb))
        for s in sorted(set(ka) ^ set(kb)):
            bad += 1; print(f"{name} {s}: only in {'A' if s in ka else 'B'}")
        for s in sorted(set(ka) & set(kb)):
            (ta, ra, ha), (tb, rb, hb) = ka[s], kb[s]
            text, regs = ta == tb, ra == rb
            hist = {k: v for k, v in ha.items() if k not in ign} == {k: v for k, v in hb.items() if k not in ign}
            n += 1; same += text; reorder += (not text and regs and hist); bad += not (regs and hist)
            if a.v or not text:
                d = [] if regs else [f"{f} {ra.get(f)}->{rb.get(f)}" for f in FIELDS if ra.get(f) != rb.get(f)]
                d += [] if hist else [f"{k} {ha[k]}->{hb[k]}" for k in sorted(set(ha) | set(hb)) if ha[k] != hb[k] and k not in ign]
                print(f"{name} {s}: text {'same' if text else 'differs'}, resources {'same' if regs else 'DIFFER'}, "
                      f"opcodes {'same' if hist else 'DIFFER'} ({sum(ha.values())}->{sum(hb.values())} instructions) {'; '.join(d)}")
    print(f"{n} kernels compared: {same} text-identical, {reorder} differ only in register naming or order, {bad} outside")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
