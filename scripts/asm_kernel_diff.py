"""Compare two device-assembly files (hipcc --cuda-device-only -S) kernel by
kernel: the same set of function names, and the same body for each once the
function number in local labels is normalised and comments (which repeat those
labels) are dropped.  For refactors that move the host functions instantiating
the kernels, so that the kernels' order in the output moves with them.

    asm_kernel_diff.py parent.s new.s      exit status 0: equal"""
import collections
import re
import sys


def norm(line):
    line = re.sub(r"BB\d+_", "BB_", line)
    line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
    return re.sub(r"\s*;.*$", "", line.rstrip("\n"))


def read(path):
    fn, cur, buf, every = {}, None, [], collections.Counter()
    for line in open(path):
        if "__hip_cuid_" in line:  # a per-file hash
            continue
        every[norm(line)] += 1
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            cur, buf = m.group(1), []
        elif cur is not None:
            if "; -- End function" in line:
                fn[cur], cur = buf, None
            else:
                buf.append(norm(line))
    return fn, every


a, la = read(sys.argv[1])
b, lb = read(sys.argv[2])
only = sorted(set(a) ^ set(b))
bad = sorted(k for k in a if k in b and a[k] != b[k])
rest = (la - lb) + (lb - la)  # everything outside the bodies too (metadata, .set lines)
print(f"{len(a)} and {len(b)} functions; {len(only)} in one file only; {len(bad)} bodies differ; "
      f"{sum(rest.values())} lines differ in the files as multisets")
for k in only + bad:
    print("  ", k)
sys.exit(1 if only or bad or rest else 0)
