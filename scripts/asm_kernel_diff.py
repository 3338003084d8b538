"""Compare device assembly (hipcc --cuda-device-only -S) kernel by kernel: the
parent's one file against the union of the new side's files.  Equal means the
same set of function names, the same body for each once the function number
in local labels is normalised and comments (which repeat those labels) are
dropped, and for each kernel the same descriptor (.amdhsa_kernel block) and
the same entry in the metadata.  For refactors that move kernels between
translation units or reorder the host functions instantiating them.

    asm_kernel_diff.py [--map OLD=NEW ...] parent.s new1.s [new2.s ...]

A kernel must stand in exactly one new file; a function that is no kernel may
stand in several, with one body.  --map rewrites OLD to NEW in the parent's
text before pairing (a kernel parameter type that changed namespace changes
the mangled names by that token); the pairing must stay one-to-one.
Exit status 0: equal."""
import re
import sys


def norm(line):
    line = re.sub(r"BB\d+_", "BB_", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    return re.sub(r"\s*;.*$", "", line.rstrip("\n"))


def read(path, maps):
    """bodies, descriptors and metadata entries by function name"""
    body, desc, meta = {}, {}, {}
    cur = buf = None  # inside a body
    dname = dbuf = None  # inside an .amdhsa_kernel block
    mbuf = None  # inside a metadata entry (a "  - .agpr_count" ... list item of amdhsa.kernels)
    in_meta = False

    def close_meta():
        nonlocal mbuf
        if mbuf:
            name = next((l.split(":", 1)[1].strip() for l in mbuf if l.strip().startswith(".name:")), None)
            if name is not None:
                meta[name] = mbuf
        mbuf = None

    for line in open(path):
        if "__hip_cuid_" in line:  # a per-file hash
            continue
        for old, new in maps:
            line = line.replace(old, new)
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            cur, buf = m.group(1), []
            continue
        s = norm(line)
        # the descriptor stands between the function's end label and its "End function" line
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", s)
        if m:
            dname, dbuf = m.group(1), []
        elif dname is not None:
            if s.strip() == ".end_amdhsa_kernel":
                desc[dname], dname = dbuf, None
            else:
                dbuf.append(s)
        if cur is not None:
            if "; -- End function" in line:
                if cur in body:
                    sys.exit(f"{path}: {cur} defined twice")
                body[cur], cur = buf, None
            else:
                buf.append(s)
            continue
        if s.strip() == "amdhsa.kernels:":
            in_meta = True
        elif in_meta:
            if re.match(r"^  - ", s):  # the next kernel's entry
                close_meta()
                mbuf = [s]
            elif re.match(r"^\S", s):  # amdhsa.target, the end of the list
                close_meta()
                in_meta = False
            elif mbuf is not None:
                mbuf.append(s)
    close_meta()
    return body, desc, meta


def main(argv):
    maps, files = [], []
    it = iter(argv)
    for a in it:
        if a == "--map":
            old, new = next(it).split("=", 1)
            maps.append((old, new))
        else:
            files.append(a)
    if len(files) < 2:
        sys.exit(__doc__)
    pb, pd, pm = read(files[0], maps)
    nb, nd, nm, where = {}, {}, {}, {}
    errors = []
    for f in files[1:]:
        b, d, m = read(f, [])
        for k, v in b.items():
            if k in nb:
                if k in d or k in nd:
                    errors.append(f"kernel {k} stands in {where[k]} and {f}")
                elif nb[k] != v:
                    errors.append(f"function {k} differs between {where[k]} and {f}")
            nb[k], where[k] = v, f
        nd.update(d)
        nm.update(m)
    # one-to-one: read() refuses a name defined twice (two parent names mapped onto one), and
    # the two sides' name sets must be equal
    only = sorted(set(pb) ^ set(nb))
    bad = sorted(k for k in pb if k in nb and pb[k] != nb[k])
    kern_only = sorted(set(pd) ^ set(nd))
    bad_desc = sorted(k for k in pd if k in nd and pd[k] != nd[k])
    bad_meta = sorted(k for k in pd if pm.get(k) != nm.get(k) or k not in pm)
    print(f"{len(pb)} and {len(nb)} functions ({len(pd)} and {len(nd)} kernels, {len(files) - 1} new files); "
          f"{len(only)} on one side only; {len(bad)} bodies differ; {len(bad_desc)} descriptors differ; "
          f"{len(bad_meta)} metadata entries differ")
    for f in files[1:]:
        print(f"   {f}: {sum(1 for k in nd if where.get(k) == f)} kernels")
    for e in errors:
        print("  ", e)
    for tag, ks in (("one side only", only), ("body", bad), ("kernel on one side only", kern_only),
                    ("descriptor", bad_desc), ("metadata", bad_meta)):
        for k in ks:
            print(f"   {tag}: {k}")
    return 1 if errors or only or bad or kern_only or bad_desc or bad_meta else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
