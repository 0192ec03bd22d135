#!/usr/bin/env python3
"""Two assembly files of one translation unit (hipcc -S --offload-device-only), kernel by kernel: the kernel descriptor's
register, spill, LDS and scratch figures, the instruction totals and every opcode whose count differs, as JSON.

    python scripts/isa_compare.py parent.s change.s out.json [--unit NAME] [--flags "..."] [--note "..."]

An instruction is a tab-indented line between a kernel's label and its s_endpgm whose first word is neither a directive
nor a comment; the histogram is over first words, whatever they are.
"""
import argparse
import collections
import json
import re

FIGURES = {"vgpr_count": ".vgpr_count", "sgpr_count": ".sgpr_count", "vgpr_spill_count": ".vgpr_spill_count",
           "sgpr_spill_count": ".sgpr_spill_count", "group_segment_fixed_size": ".group_segment_fixed_size",
           "private_segment_fixed_size": ".private_segment_fixed_size"}


def kernels(path):
    """{symbol: (descriptor figures, Counter of opcodes)} of every kernel of an assembly file"""
    text = open(path).read()
    meta = {}
    for block in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):])[1:]:  # (a kernel's arguments are indented deeper)
        name = re.search(r"\n    \.name:\s+(\S+)", block)
        if name:
            meta[name.group(1)] = {k: int(re.search(re.escape(v) + r":\s+(\d+)", block).group(1)) for k, v in FIGURES.items()}
    out = {}
    for name, figures in meta.items():
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M).group(1)
        words = [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and ln.split()]
        out[name] = (figures, collections.Counter(w for w in words if w[0] not in ".;"))
    return out


def main():
    pa = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    pa.add_argument("parent")
    pa.add_argument("change")
    pa.add_argument("out")
    pa.add_argument("--unit", default=None)
    pa.add_argument("--flags", default="")
    pa.add_argument("--note", default="")
    args = pa.parse_args()
    a, b = kernels(args.parent), kernels(args.change)
    report = {"flags": args.flags.split(), "note": args.note, "same_kernel_symbols": sorted(a) == sorted(b),
              "only_in_parent": sorted(set(a) - set(b)), "only_in_change": sorted(set(b) - set(a)), "kernels_that_differ": [],
              "kernels": {}}
    for name in sorted(set(a) & set(b)):
        (fa, ca), (fb, cb) = a[name], b[name]
        diff = {op: [ca[op], cb[op]] for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]}
        if diff or fa != fb:
            report["kernels_that_differ"].append(name)
        report["kernels"][name] = {"unit": args.unit, "parent": fa, "change": fb,
                                   "instructions": [sum(ca.values()), sum(cb.values())], "opcode_counts_that_differ": diff}
    json.dump(report, open(args.out, "w"), indent=1)
    print("%d kernels, %d differ: %s" % (len(report["kernels"]), len(report["kernels_that_differ"]),
                                         ", ".join(report["kernels_that_differ"]) or "none"))


if __name__ == "__main__":
    main()
