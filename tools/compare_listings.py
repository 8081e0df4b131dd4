#!/usr/bin/env python3
"""Are the kernels of one build of rt_analyze.hip unchanged in another?  Two `hipcc -S --cuda-device-only` listings made with the
product's flags (pyradiotracking_amd/build.py), matched by demangled kernel name; a kernel's machine code is its text from its label
to its end label, the .amdhsa_kernel descriptor included, with the per-function numbers of local labels taken out (a kernel added in
front renumbers them).

    tools/compare_listings.py before.s after.s

Prints the counts (identical / changed / removed / added, the added ones by family) and the names of changed or removed kernels;
exit status 1 if any kernel of `before` is changed or missing."""
import collections
import re
import subprocess
import sys


def kernels(path):
    out, name, body, is_kernel = {}, None, [], False
    for ln in open(path, errors="replace"):
        if name is None:
            m = re.match(r"([A-Za-z_][^\s:]*):", ln)
            if m:
                name, body, is_kernel = m.group(1), [], False
            continue
        if ln.startswith(".Lfunc_end"):
            if is_kernel:
                out[name] = "".join(body)
            name = None
            continue
        if ln.lstrip().startswith(".amdhsa_kernel "):
            is_kernel = True
        ln = re.sub(r";.*", "", ln).rstrip()  # comments (they carry block numbers; the padding in front of them varies with the numbers' width)
        body.append(re.sub(r"\.L(BB|tmp)\d+", r".L\1", ln) + "\n")
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, r))


def main():
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangle(sorted(set(before) | set(after)))
    same = [n for n in before if n in after and before[n] == after[n]]
    changed = [n for n in before if n in after and before[n] != after[n]]
    removed = [n for n in before if n not in after]
    added = [n for n in after if n not in before]
    print(f"kernels before {len(before)}, after {len(after)}: identical {len(same)}, changed {len(changed)}, removed {len(removed)}, added {len(added)}")
    fam = collections.Counter(re.sub(r"^void rt::|<.*", "", names[n]) for n in added)
    for k, v in sorted(fam.items()):
        print(f"  added {k}: {v}")
    for n in changed:
        print("  CHANGED", names[n])
    for n in removed:
        print("  REMOVED", names[n])
    return 1 if changed or removed else 0


if __name__ == "__main__":
    sys.exit(main())
