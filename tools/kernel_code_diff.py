#!/usr/bin/env python3
"""Compares two device assembly listings of libppo_hip kernel by kernel: the proof that a refactor left the machine code alone.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S -I include ppo_cpp_amd/csrc/ppo_hip.hip -o a.s     (both trees)
    python tools/kernel_code_diff.py a.s b.s

Prints the kernels that only one listing has, the kernels whose instruction stream differs (instruction counts, changed lines, whether the
opcodes are the same multiset) and the kernels whose metadata figures (registers, LDS, kernarg, scratch, spills) differ.  Comments and
directives are dropped and basic-block labels renumbered in order of appearance before the comparison.  Exit status 1 when anything differs.
It compares two listings and nothing else."""
import collections
import difflib
import re
import shutil
import subprocess
import sys

FIGURES = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "kernarg_segment_size", "private_segment_fixed_size",
           "vgpr_spill_count", "sgpr_spill_count")
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def parse(text):
    """{kernel: (instruction stream, metadata figures)}; a stream line is an instruction or a renumbered label."""
    lines = text.splitlines()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    code, cur, labels = {}, None, {}
    for raw in lines:
        line = re.split(r";|//", raw, 1)[0].strip()
        m = re.fullmatch(r"([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in kernels:
            cur, labels = code.setdefault(m.group(1), []), {}
            continue
        if cur is None or not line:
            continue
        if line.startswith(".amdhsa_kernel") or line.startswith(".Lfunc_end"):
            cur = None
        elif line.endswith(":") or not line.startswith("."):                     # a label or an instruction: directives go
            cur.append(LABEL.sub(lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), " ".join(line.split())))
    meta, name, fig = {}, None, {}
    for raw in lines[lines.index("amdhsa.kernels:") + 1 if "amdhsa.kernels:" in lines else len(lines):]:
        if not raw.startswith("  "):
            break
        if raw.startswith("  - "):                                               # the next kernel's entry
            if name: meta[name] = fig
            name, fig = None, {}
        m = re.fullmatch(r"  [ -] \.(\w+):\s*(\S+)", raw)
        if m and m.group(1) == "name": name = m.group(2)
        elif m and m.group(1) in FIGURES: fig[m.group(1)] = int(m.group(2))
    if name: meta[name] = fig
    return {k: (code.get(k, []), meta.get(k, {})) for k in kernels}


def compare(a, b):
    """a, b: parse() results.  -> {"only_a", "only_b": names; "code": {name: figures of the difference}; "meta": {name: {key: (a, b)}}; "same": count}"""
    rep = {"only_a": sorted(set(a) - set(b)), "only_b": sorted(set(b) - set(a)), "code": {}, "meta": {}, "same": 0}
    for k in sorted(set(a) & set(b)):
        (ca, ma), (cb, mb) = a[k], b[k]
        if ca != cb:
            ia, ib = [l for l in ca if not l.endswith(":")], [l for l in cb if not l.endswith(":")]
            d = [l for l in difflib.unified_diff(ca, cb, lineterm="", n=0) if l[0] in "+-" and not l.startswith(("+++", "---"))]
            rep["code"][k] = {"instructions": (len(ia), len(ib)), "removed": sum(l[0] == "-" for l in d), "added": sum(l[0] == "+" for l in d),
                              "same_opcodes": collections.Counter(l.split()[0] for l in ia) == collections.Counter(l.split()[0] for l in ib)}
        if ma != mb:
            rep["meta"][k] = {f: (ma.get(f), mb.get(f)) for f in FIGURES if ma.get(f) != mb.get(f)}
        if ca == cb and ma == mb:
            rep["same"] += 1
    return rep


def demangle(names):
    if not names or not shutil.which("c++filt"):
        return {n: n for n in names}
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return {n: re.sub(r"\(.*", "", o).replace("void ", "") for n, o in zip(names, out)}


def report(rep, na, nb):
    names = demangle(rep["only_a"] + rep["only_b"] + sorted(set(rep["code"]) | set(rep["meta"])))
    out = ["kernels: %d in A, %d in B; %d in both with identical instruction stream and metadata figures" % (na, nb, rep["same"])]
    out += ["only in A: " + names[k] for k in rep["only_a"]] + ["only in B: " + names[k] for k in rep["only_b"]]
    for k, d in rep["code"].items():
        out.append("code differs: %s: instructions %d -> %d, lines -%d +%d, %s" % (names[k], d["instructions"][0], d["instructions"][1], d["removed"], d["added"],
                                                                                   "same opcode multiset" if d["same_opcodes"] else "other opcodes"))
    for k, d in rep["meta"].items():
        out.append("metadata differs: %s: %s" % (names[k], ", ".join("%s %s -> %s" % (f, v[0], v[1]) for f, v in d.items())))
    return "\n".join(out)


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = parse(open(argv[1]).read()), parse(open(argv[2]).read())
    rep = compare(a, b)
    print(report(rep, len(a), len(b)))
    return 1 if rep["only_a"] or rep["only_b"] or rep["code"] or rep["meta"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
