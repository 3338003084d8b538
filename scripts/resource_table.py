#!/usr/bin/env python3
"""The layer kernels' lines of a resource table (profiles/r21/resource_usage.txt)
from one compile each of the files that hold the layer kernels, cbic_layers.hip
and cbic_layers_cons.hip:

    hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage \
        -o cbic_layers.s urlearning-cpp_amd/csrc/cbic_layers.hip 2> cbic_layers_ru.log
    (the same for cbic_layers_cons)
    python scripts/resource_table.py cbic_layers_ru.log cbic_layers_cons_ru.log \
        cbic_layers.s cbic_layers_cons.s [LAYERS, default 4,5,6]

Any number of remark logs and of assembly files (*.s), in any order.

One line per score_layer_kernel / score_layer_cons_kernel instantiation of the
given layers, the remarks' numbers in profiles/r16's layout; with the assembly,
the layer-6 two-pass kernels also get their static instruction counts: VALU
(mnemonics v_*), of which FP64 (*_f64), scratch loads and stores, and the
find-first-bit instructions of the element extraction (v_ffbl_*).
"""
import re
import sys

NAME = re.compile(r"score_layer(_cons)?_kernelILi(\d+)ELi(\d+)ELi(\d+)E(?:Lb([01])E)?")


def label(m):
    cons, L, ph, V, nw = m.groups()
    return "score_layer%s_kernel<%s,%s,%s%s>" % (cons or "", L, ph, V, "" if nw is None else (",narrow" if nw == "1" else ",wide"))


def remarks(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            k = NAME.search(m.group(1))
            cur = label(k) if k else None
            if cur:
                out[cur] = {"key": tuple(int(x or 0) for x in (k.group(1) is not None, k.group(2), k.group(3), k.group(4), k.group(5)))}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def static_counts(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            k = NAME.search(m.group(1))
            cur = label(k) if k else None
            if cur:
                out[cur] = dict(valu=0, f64=0, scratch_ld=0, scratch_st=0, ffbl=0)
            continue
        if "; -- End function" in line:
            cur = None
        if not cur:
            continue
        t = line.split()
        if not t or t[0].startswith((";", ".", "BB")) or t[0].endswith(":"):
            continue
        op = t[0]
        c = out[cur]
        if op.startswith("v_"):
            c["valu"] += 1
            c["f64"] += "_f64" in op
            c["ffbl"] += op.startswith("v_ffbl")
        c["scratch_ld"] += op.startswith("scratch_load")
        c["scratch_st"] += op.startswith("scratch_store")
    return out


def main():
    ru, st, layers = {}, {}, [4, 5, 6]
    for a in sys.argv[1:]:
        if re.fullmatch(r"\d+(,\d+)*", a):
            layers = [int(x) for x in a.split(",")]
        elif a.endswith(".s"):
            st.update(static_counts(a))
        elif a != "-":
            ru.update(remarks(a))
    for name, r in sorted(ru.items(), key=lambda kv: kv[1]["key"]):
        if r["key"][1] not in layers:
            continue
        line = "%s TotalSGPRs=%s VGPRs=%s AGPRs=%s ScratchSize=%s Occupancy=%s" % (
            name, r["TotalSGPRs"], r["VGPRs"], r["AGPRs"], r["ScratchSize"], r["Occupancy"])
        s = st.get(name)
        if s and r["key"][1] == 6 and r["key"][3] == 209:
            line += "  static: VALU=%d (FP64 %d) scratch_load=%d scratch_store=%d v_ffbl=%d" % (
                s["valu"], s["f64"], s["scratch_ld"], s["scratch_st"], s["ffbl"])
        print(line)


if __name__ == "__main__":
    main()
