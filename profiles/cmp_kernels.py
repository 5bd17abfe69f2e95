"""Compares the kernels of two sets of `hipcc --cuda-device-only -S` outputs, kernel by kernel.

    python profiles/cmp_kernels.py OLD.s [OLD.s ...] -- NEW.s [NEW.s ...]

Each file is split at its kernel symbols (the `.amdhsa_kernel` names: the text from `<name>:` to the
function's `.Lfunc_end`), local labels (`.LBB<fn>_<n>`, `.Ltmp<n>`, `.Lfunc_*`) are renamed in order of
appearance inside the kernel, comments and blank lines are dropped, and the instruction text of every
kernel name is compared between the two sets: the kernels may be spread differently over the files of each
side.  Prints the counts and every kernel that is missing, extra or different; exit status 1 if any is.
"""
import re
import sys

LABEL = re.compile(r"\.L(?:BB\d+_\d+|tmp\d+|func_(?:begin|end)\d+)")


def kernels(path):
    lines = open(path).read().split("\n")
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    out, name, body, seen = {}, None, [], {}
    for ln in lines:
        m = re.match(r"(\S+):", ln)
        if name is None:
            if m and m.group(1) in names:
                name, body, seen = m.group(1), [], {}
            continue
        if re.match(r"\.Lfunc_end\d+:", ln):
            out[name] = body
            name = None
            continue
        ln = ln.split(";")[0].strip()
        if not ln or ln.startswith(".loc") or ln.startswith(".file") or ln.startswith(".cfi"):
            continue
        body.append(LABEL.sub(lambda q: seen.setdefault(q.group(0), ".L%d" % len(seen)), ln))
    return out


def collect(paths):
    all_k = {}
    for p in paths:
        for n, b in kernels(p).items():
            if n in all_k:
                sys.exit(f"kernel {n} appears twice on one side ({p})")
            all_k[n] = b
    return all_k


def main(argv):
    if "--" not in argv:
        sys.exit(__doc__)
    i = argv.index("--")
    old, new = collect(argv[:i]), collect(argv[i + 1:])
    missing = sorted(set(old) - set(new))
    extra = sorted(set(new) - set(old))
    differ = sorted(n for n in set(old) & set(new) if old[n] != new[n])
    print(f"old: {len(old)} kernels, new: {len(new)} kernels, equal: {len(set(old) & set(new)) - len(differ)}")
    for tag, names in (("missing", missing), ("extra", extra), ("differs", differ)):
        for n in names:
            print(f"{tag}: {n}")
    return 1 if (missing or extra or differ) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
