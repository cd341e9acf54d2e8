#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel in two device assembly files.

    hipcc <the flags _build.py uses for the file> --cuda-device-only -S file.hip -o file.s
    python tools/asm_kernel_diff.py old.s new.s [--markdown] [--show NAME]

For a refactor that must not change generated code: the kernels of both files are paired by
demangled name and, per pair, the instruction text and the .amdhsa_* block (register counts,
scratch, LDS) are compared after comments and debug directives are stripped and local labels
renumbered in order of appearance.  Several files of one tree (a translation unit that was split)
can be concatenated into one argument file.  Exit status 1 if a kernel is missing, new or differs.

--map OLD=NEW rewrites a demangled name of the first file before pairing (a regular expression
and its replacement), e.g. --map 'k_c3x6p<(.*), 8>=k_c3x6p<\\1>' for a dropped template argument.
"""
from __future__ import annotations

import argparse
import difflib
import re
import subprocess
import sys

CXXFILT = "c++filt"
LABEL = re.compile(r"\.L[A-Za-z_]+[0-9][0-9_]*")
DROP = re.compile(r"^\s*\.(loc|file|cfi_\w+|ident|section|addrsig\w*)\b")


def demangle(names: list[str]) -> list[str]:
    out = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True)
    return out.stdout.split("\n")[: len(names)]


def normalise(lines: list[str], sym: str) -> list[str]:
    labels: dict[str, str] = {}

    def relabel(m: re.Match) -> str:
        return labels.setdefault(m.group(0), f".L{len(labels)}")

    out = []
    for ln in lines:
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or DROP.match(ln):
            continue
        # the kernel's own name inside its symbols (its LDS arrays): paired kernels may mangle apart
        ln = ln.replace(sym[2:], "SELF")
        out.append(LABEL.sub(relabel, " ".join(ln.split())))
    return out


def kernels(path: str) -> dict[str, tuple[list[str], list[str]]]:
    """demangled name -> (normalised body, normalised .amdhsa block)"""
    text = open(path).read().split("\n")
    syms = [m.group(1) for ln in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    res = {}
    for sym, name in zip(syms, demangle(syms)):
        beg = next(i for i, ln in enumerate(text) if ln.split(";", 1)[0].rstrip() == sym + ":")
        end = next(i for i in range(beg, len(text)) if text[i].startswith(".Lfunc_end"))
        h0 = next(i for i, ln in enumerate(text) if re.match(rf"\s*\.amdhsa_kernel\s+{re.escape(sym)}$", ln))
        h1 = next(i for i in range(h0, len(text)) if ".end_amdhsa_kernel" in text[i])
        name = re.sub(r"^void ", "", name)
        assert name not in res, f"{path}: {name} twice"
        res[name] = (normalise(text[beg + 1:end], sym), normalise(text[h0 + 1:h1], sym))
    return res


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--markdown", action="store_true", help="print the table as markdown")
    ap.add_argument("--show", metavar="NAME", help="unified diff of the kernels whose name contains NAME")
    args = ap.parse_args()
    old, new = kernels(args.old), kernels(args.new)
    for m in args.map:
        pat, repl = m.split("=", 1)
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    bad = 0
    rows = []
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            rows.append((name, "missing in new" if name in old else "new"))
            bad += 1
            continue
        code = old[name][0] == new[name][0]
        meta = old[name][1] == new[name][1]
        rows.append((name, "yes" if code and meta else "no (" + ", ".join(
            w for w, ok in (("code", code), ("amdhsa", meta)) if not ok) + ")"))
        bad += not (code and meta)
        if args.show and args.show in name and not (code and meta):
            for k in (0, 1):
                sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(
                    old[name][k], new[name][k], "old " + name, "new " + name, lineterm="", n=2))
    if args.markdown:
        print("| kernel | identical |\n|---|---|")
    for name, verdict in rows:
        print(f"| `{name}` | {verdict} |" if args.markdown else f"{verdict:16s} {name}")
    print(f"{len(rows)} kernels, {len(rows) - bad} identical, {bad} not", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
