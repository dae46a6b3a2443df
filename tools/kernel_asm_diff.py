"""Compare the machine code of two builds function by function: every kernel and every out-of-line device function of the given assembly files
(hipcc <build.py's flags> --offload-device-only -S), by instruction stream and, for kernels, by the resource metadata vgpr_count, sgpr_count,
agpr_count, group_segment_fixed_size and private_segment_fixed_size.  What a moved function legitimately changes is normalised first: local label
numbers and the order of the symbols (functions are matched by name, across files).

    python tools/kernel_asm_diff.py OLD.s [OLD2.s ...] -- NEW.s [NEW2.s ...]

Prints one line per function, "identical" or what differs; exit status 1 if anything differs or a function exists on one side only."""
import re
import sys

META_KEYS = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def functions(text):
    """name -> normalised instruction lines"""
    out, name, body = {}, None, []
    types = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    for line in text.split("\n"):
        m = re.match(r"^(\S+):", line)
        if name is None:
            if m and m.group(1) in types:
                name, body = m.group(1), []
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            out[name] = normalise(body)
            name = None
            continue
        body.append(line)
    return out


def normalise(lines):
    labels, res = {}, []

    def local(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))

    for line in lines:
        line = line.split(";")[0].rstrip()
        if not line.strip() or re.match(r"^\s*\.(p2align|loc|file|cfi_|section|text)", line):
            continue
        res.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)[0-9_]+", local, " ".join(line.split())))
    return res


def metadata(text):
    """kernel name -> the META_KEYS of its entry in the amdgpu metadata"""
    entries = []
    for line in text.split("\n"):
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            entries.append({})
        if entries:
            entries[-1][m.group(2)] = m.group(3).strip()
    return {e["name"]: tuple(e.get(k) for k in META_KEYS) for e in entries if "symbol" in e}


def load(paths):
    funcs, meta = {}, {}
    for p in paths:
        text = open(p).read()
        funcs.update(functions(text))
        meta.update(metadata(text))
    return funcs, meta


def main(argv):
    cut = argv.index("--")
    (fa, ma), (fb, mb) = load(argv[:cut]), load(argv[cut + 1:])
    bad = 0
    for name in sorted(set(fa) | set(fb)):
        kind = "kernel  " if name in ma or name in mb else "function"
        if name not in fa or name not in fb:
            verdict = "only in the %s build" % ("old" if name in fa else "new")
        elif fa[name] != fb[name]:
            first = next((i for i, (x, y) in enumerate(zip(fa[name], fb[name])) if x != y), min(len(fa[name]), len(fb[name])))
            verdict = "instructions differ (%d / %d lines, first at %d)" % (len(fa[name]), len(fb[name]), first)
        elif ma.get(name) != mb.get(name):
            verdict = "metadata differ: %s / %s" % (ma.get(name), mb.get(name))
        else:
            verdict = "identical" + (" (%d instructions; %s)" % (len(fa[name]), ", ".join("%s %s" % kv for kv in zip(META_KEYS, ma[name]))) if name in ma else "")
        bad += not verdict.startswith("identical")
        print("%s %s: %s" % (kind, name, verdict))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
