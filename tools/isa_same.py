"""Are the functions of two sets of assembly listings the same machine code?

usage: python tools/isa_same.py PARENT.s [PARENT2.s ...] -- THIS.s [THIS2.s ...] [--must-match REGEX]

The listings are what `make -C small-pathtracer_amd/csrc isa` writes (hipcc -S, device only). Functions
are matched by mangled name across all files of a side, so code may move between files. Two things
are compared per function, both as plain strings:

  * its text, from its label to its .Lfunc_end, comments stripped and the function's ordinal in its
    file masked in the block labels (BB<n>_), which is all that moves when a function does;
  * its .amdhsa_kernel descriptor block (registers, LDS, scratch), for a kernel.

One line per function: identical, differs (with both line counts), only in the parent, or only here.
The exit status is 0 only if every function whose name matches --must-match is on both sides and
identical on both counts; without --must-match, every function present on both sides.
"""
import re
import sys

_TYPE = re.compile(r"^\s*\.type\s+([^\s,]+),@function")
_ORDINAL = re.compile(r"BB\d+_")


def _clean(line):
    return _ORDINAL.sub("BB#_", line.split(";", 1)[0]).strip()


def functions(text):
    """{mangled name: (text lines, descriptor lines or None)} of one listing."""
    lines = text.splitlines()
    names = [m.group(1) for m in map(_TYPE.match, lines) if m]
    out = {}
    for name in names:
        start = next((i for i, ln in enumerate(lines) if ln.startswith(name + ":")), None)
        if start is None:
            continue  # declared, not defined here
        body = []
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            c = _clean(ln)
            if c:
                body.append(c)
        desc, head = None, ".amdhsa_kernel " + name
        for i, ln in enumerate(lines):
            if ln.strip() == head:
                end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
                desc = [c for c in map(_clean, lines[i + 1:end]) if c]
                break
        out[name] = (body, desc)
    return out


def side(paths):
    out = {}
    for p in paths:
        with open(p) as f:
            fs = functions(f.read())
        dup = sorted(set(fs) & set(out))
        if dup:
            raise SystemExit(f"{p}: {dup[0]} is defined in two listings of one side")
        out.update(fs)
    return out


def compare(parent, here, must_match=None):
    """(report lines, exit status)."""
    rx = re.compile(must_match) if must_match else None
    report, bad, named = [], 0, 0
    for name in sorted(set(parent) | set(here)):
        must = bool(rx.search(name)) if rx else (name in parent and name in here)
        named += must
        if name not in here:
            verdict = "only in the parent"
        elif name not in parent:
            verdict = "only here"
        else:
            (pt, pd), (ht, hd) = parent[name], here[name]
            if pt == ht and pd == hd:
                verdict = "identical"
            else:
                what = [w for w, same in (("text", pt == ht), ("descriptor", pd == hd)) if not same]
                verdict = f"differs ({' and '.join(what)}; parent {len(pt)} lines, here {len(ht)})"
        if must and verdict != "identical":
            bad += 1
        report.append(f"{verdict:20s} {name}")
    if rx and not named:
        report.append(f"no function matches {must_match!r}")
        bad += 1
    report.append(f"{named} functions had to match, {bad} did not")
    return report, 1 if bad else 0


def main(argv):
    must = None
    args = []
    it = iter(argv)
    for a in it:
        if a == "--must-match":
            must = next(it, None)
        elif a.startswith("--must-match="):
            must = a.split("=", 1)[1]
        else:
            args.append(a)
    if "--" not in args or must == "":
        raise SystemExit(__doc__)
    k = args.index("--")
    parent, here = args[:k], args[k + 1:]
    if not parent or not here or (must is None and "--must-match" in argv):
        raise SystemExit(__doc__)
    report, status = compare(side(parent), side(here), must)
    print("\n".join(report))
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
