"""The activation arena in numbers, on the host alone (grnet_arena_query / grnet_arena_layout touch no device): per precision and for
max_frames in {16, 64, 400, 2048} the bytes of the default (full) layout, of the compact layout (GRNET_CREATE_COMPACT_ARENA) and the lower
bound of any layout under the sharing rule; the ten largest tensors with their co-tenants; and the stack of tensors under the arena's top,
which says what the distance to the bound is spent on.

    python tools/arena_report.py [out.md]         # profiles/arena_layout.md is this tool's output, written whole
"""
import ctypes as C
import importlib
import os
import sys

SIZES = (16, 64, 400, 2048)
COMPACT = 1


def up(x, a=64):
    return (x + a - 1) // a * a


def layout(lib, precision, max_frames, flags):
    need = lib.grnet_arena_layout(precision, max_frames, flags, None, 0)
    assert need > 0, need
    buf = C.create_string_buffer(need)
    assert lib.grnet_arena_layout(precision, max_frames, flags, buf, need) == need - 1
    tensors, ops, groups = {}, [], []
    for f in (line.split() for line in buf.value.decode().splitlines()):
        if f[0] == "tensor":
            tensors[int(f[1])] = (f[2], int(f[3]), int(f[4]))
        elif f[0] == "op":
            w = f.index("writes")
            ops.append((f[2], [int(x) for x in f[4:w]], [int(x) for x in f[w + 1:]]))
        elif f[0] == "group":
            groups.append([int(x) for x in f[1:]])
    return tensors, ops, groups


def conflicts(tensors, ops, groups):
    """The sharing rule restated: a, b conflict unless every op touching one is a strict ancestor (RAW DAG) of every op writing the other;
    and whatever a launch group writes conflicts with whatever it touches."""
    anc, writers, touch = [], {}, {}
    for i, (_, rd, wr) in enumerate(ops):
        a = 0
        for t in rd:
            for w in writers.get(t, ()):
                a |= anc[w] | 1 << w
        anc.append(a)
        for t in wr:
            writers.setdefault(t, []).append(i)
        for t in rd + wr:
            touch.setdefault(t, set()).add(i)

    def earlier(a, b):
        return bool(touch.get(a)) and bool(writers.get(b)) and all(x != w and (anc[w] >> x) & 1 for x in touch[a] for w in writers[b])
    ids = sorted(tensors)
    conf = {(a, b) for a in ids for b in ids if a < b and not earlier(a, b) and not earlier(b, a)}
    for g in groups:
        wr = {t for i in g for t in ops[i][2]}
        tc = wr | {t for i in g for t in ops[i][1]}
        conf |= {(min(a, b), max(a, b)) for a in wr for b in tc if a != b}
    return conf, earlier


def describe(tensors, k):
    name, per_frame, _ = tensors[k]
    return f"{name}#{k}" if name != "-" else f"#{k}"


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    pkg = importlib.import_module("video-based-gait-analysis-for-dementia_amd")
    lib = pkg._lib.load()
    out = ["# Activation arena: full and compact layouts", "",
           "Written by `tools/arena_report.py` (host only: `grnet_arena_query`, `grnet_arena_layout`).  Bytes include the 256-byte zero block in front",
           "and the 256 bytes of tail.  *bound*: the largest sum of tensors alive across one launch (written by it or before it, used by it or after it), over",
           "every op and every launch group; no layout under the sharing rule of `DESIGN.md` section 3 is smaller.  *compact / bound* is a measurement.", ""]
    for precision, pname in ((0, "fp32"), (1, "bf16")):
        out += [f"## {pname}", "", "| max_frames | full bytes | compact bytes | bound bytes | full / compact | compact / bound | tensors | sharing |", "|---:|---:|---:|---:|---:|---:|---:|---:|"]
        for m in SIZES:
            info = (C.c_int64 * 5)()
            assert lib.grnet_arena_query(precision, m, COMPACT, info) == 0
            comp, full, bound, nt, shared = (int(v) for v in info)
            out.append(f"| {m} | {full:,} | {comp:,} | {bound:,} | {full / comp:.2f} | {comp / bound:.3f} | {nt} | {shared} |")
        m = 64
        tensors, ops, groups = layout(lib, precision, m, COMPACT)
        conf, earlier = conflicts(tensors, ops, groups)
        size = {k: up(t[1] * m) for k, t in tensors.items()}
        rng = {k: (t[2], t[2] + size[k]) for k, t in tensors.items()}
        out += ["", f"Per frame: full {sum(t[1] for t in tensors.values()) * 4 / 1e6:.1f} MB, compact {(max(r[1] for r in rng.values()) - 64) * 4 / m / 1e6:.1f} MB "
                f"({len(ops) - 1} ops, {len(groups)} launch groups).", "",
                "The ten largest tensors (floats per frame; offset in floats per frame behind the zero block) and the tensors that share bytes with them, earlier tenants first:", "",
                "| tensor | floats / frame | offset / frame | co-tenants |", "|---|---:|---:|---|"]
        for k in sorted(tensors, key=lambda k: (-tensors[k][1], k))[:10]:
            co = [o for o in tensors if o != k and rng[o][0] < rng[k][1] and rng[k][0] < rng[o][1]]
            assert all((min(k, o), max(k, o)) not in conf for o in co)
            before = [describe(tensors, o) for o in co if earlier(o, k)]
            after = [describe(tensors, o) for o in co if not earlier(o, k)]
            short = lambda names: ", ".join(names[:6]) + (f", ... ({len(names)})" if len(names) > 6 else "")
            later = (" ; then: " + short(after)) if after else ""
            out.append(f"| {describe(tensors, k)} | {tensors[k][1]:,} | {(tensors[k][2] - 64) // m:,} | {short(before) or '-'}{later} |")
        # the stack under the top of the arena: each tensor sits on a conflicting one that ends where it starts
        top = max(tensors, key=lambda k: (rng[k][1], -k))
        stack = [top]
        while rng[stack[-1]][0] > 64:
            k = stack[-1]
            below = [o for o in tensors if rng[o][1] == rng[k][0] and (min(k, o), max(k, o)) in conf]
            if not below:
                break
            stack.append(max(below, key=lambda o: size[o]))
        clique = all((min(a, b), max(a, b)) in conf for i, a in enumerate(stack) for b in stack[i + 1:])
        out += ["", "The stack that ends at the arena's top (each tensor conflicts with the one it stands on): " +
                " / ".join(f"{describe(tensors, k)} ({tensors[k][1]:,})" for k in stack) +
                f" = {sum(tensors[k][1] for k in stack):,} floats per frame.  These {len(stack)} tensors " +
                ("conflict pairwise, so no layout under the rule is smaller than their sum: the assignment is at the optimum, and the distance to the bound is the "
                 "bound's -- it counts what is alive across ONE launch, while launches on parallel branches (the three upsample heads beside `cat`) are unordered and "
                 "conflict with each other as well." if clique else
                 "do not all conflict pairwise: first fit left a gap that another order could close.")]
        out.append("")
    text = "\n".join(out) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
