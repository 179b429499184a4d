#!/usr/bin/env python
"""Two device assemblies of csrc/trlda_hip.hip, kernel by kernel: is a refactor the same code?

    python tools/asm_compare.py PARENT.s NEW.s [name-substring ...]     (no GPU)

Each .s is what tools/sgpr_spill_scan.py compiles (hipcc -O3 -S --cuda-device-only).  A kernel whose
name holds one of the substrings is expected to differ and gets a row of parent -> new values: VGPRs
(arch + AGPR = total), SGPRs, scratch bytes, the compiler's occupancy, instructions and MFMAs.  Every
other kernel must have the same instruction text, comments and label numbers aside; those that do not
are listed.  Exit status 1 when an unexpected kernel differs, a kernel is missing on one side, or an
expected one breaks a bar: scratch > 0, another MFMA count, a total VGPR count in a higher block of
64, a lower occupancy, or an instruction count more than 3 % from the parent's.
"""
import re
import sys

from sgpr_spill_scan import kernels

INFO = {"vgpr": "NumVgprs", "agpr": "NumAgprs", "total": "TotalNumVgprs", "sgpr": "TotalNumSgprs",
        "scratch": "ScratchSize", "occupancy": "Occupancy"}


def read(path):
    lines = open(path).read().split("\n")
    out = {}
    for name, body in kernels(lines):
        ins = []
        for l in body:
            t = l.split(";")[0].strip()
            if t and not t.startswith(".") or re.match(r"^\.LBB\w+:", t):
                ins.append(re.sub(r"\.L(BB|JTI|tmp)?\d+_", ".L_", t))
        out[name] = {"text": ins, "instructions": sum(not t.endswith(":") for t in ins),
                     "mfma": sum(t.startswith("v_mfma") for t in ins)}
    name = None
    for l in lines:
        m = re.match(r"\s*\.size\s+(\w+), \.Lfunc_end", l)
        if m:
            name = m.group(1)
        for key, tag in INFO.items():
            m = re.match(r"; %s: (\d+)" % tag, l)
            if m and name in out:
                out[name][key] = int(m.group(1))
    return {n: k for n, k in out.items() if "occupancy" in k}    # kernels, not device functions


def main():
    old, new = read(sys.argv[1]), read(sys.argv[2])
    pats = sys.argv[3:]
    bad = sorted(set(old) ^ set(new))
    for n in bad:
        print("only on one side: %s" % n)
    same = 0
    for n in sorted(set(old) & set(new)):
        o, w = old[n], new[n]
        if not any(p in n for p in pats):
            if o["text"] == w["text"]:
                same += 1
            else:
                bad.append(n)
                print("DIFFERS: %s" % n)
            continue
        fails = []
        if w["scratch"] > 0:
            fails.append("scratch")
        if w["mfma"] != o["mfma"]:
            fails.append("MFMA count")
        if (w["total"] + 63) // 64 > (o["total"] + 63) // 64 or w["occupancy"] < o["occupancy"]:
            fails.append("occupancy step")
        if abs(w["instructions"] - o["instructions"]) > 0.03 * o["instructions"]:
            fails.append("instructions")
        bad += fails
        print("%s\n    vgpr %d + %d = %d -> %d + %d = %d, sgpr %d -> %d, scratch %d -> %d, occupancy %d -> %d, "
              "instructions %d -> %d (%+.1f %%), MFMA %d -> %d  %s"
              % (n, o["vgpr"], o["agpr"], o["total"], w["vgpr"], w["agpr"], w["total"], o["sgpr"], w["sgpr"],
                 o["scratch"], w["scratch"], o["occupancy"], w["occupancy"], o["instructions"], w["instructions"],
                 100.0 * (w["instructions"] - o["instructions"]) / o["instructions"], o["mfma"], w["mfma"],
                 "FAILS: " + ", ".join(fails) if fails else "ok"))
    print("%d other kernels identical" % same)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
