"""Resources and per-mnemonic instruction histogram of every kernel of one translation unit, from its device assembly:
  hipcc <build.py's FLAGS> --cuda-device-only -S csrc/wgrad.hip -o new.s        (likewise old.s from the parent commit)
  python profiles/kernel_histogram.py old.s new.s [old_name=new_name ...]
prints one row per kernel, parent beside result, and the mnemonics whose counts differ (profiles/wgrad_units_resources.txt).
A renamed or merged kernel is matched with old_name=new_name (demangled, as printed in the first column)."""
import collections
import re
import subprocess
import sys

FIELDS = [("V", ".vgpr_count"), ("A", ".agpr_count"), ("S", ".sgpr_count"), ("scratch", ".private_segment_fixed_size"),
          ("spillV", ".vgpr_spill_count"), ("spillS", ".sgpr_spill_count"), ("LDS", ".group_segment_fixed_size")]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"^\(anonymous namespace\)::|\(.*\)$|^void ", "", re.sub(r"^void \(anonymous namespace\)::", "", d)) for d in out[:len(names)]]


def read(path):
    text = open(path).read()
    res = {}
    for entry in text.split("  - .agpr_count:")[1:]:   # amdhsa.kernels metadata, one entry per kernel
        entry = ".agpr_count:" + entry
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        res[name] = {k: int(re.search(re.escape(f) + r":\s+(\d+)", entry).group(1)) for k, f in FIELDS}
    for name in res:
        body = text[re.search(rf"^{re.escape(name)}:", text, re.M).end():]
        body = body[:body.index(".Lfunc_end")]
        ops = [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and ln[1] not in ".;"]
        res[name]["hist"] = collections.Counter(ops)
        res[name]["insts"] = len(ops)
        res[name]["loop"] = chunk_loop(body.split("\n"))
    return dict(zip(demangle(list(res)), res.values()))


def chunk_loop(lines):
    """Histogram of the chunk loop: the smallest loop (by the compiler's own loop comments on the block labels) that holds
    matrix instructions, from its first block to the last branch back into it."""
    loops = collections.defaultdict(dict)   # header -> {label: line}
    for i, ln in enumerate(lines):
        m = re.match(r"(\.LBB\d+_(\d+)):\s*;.*?(?:Header=BB\d+_(\d+)|Loop Header)", ln)
        if m:
            loops[m.group(3) or m.group(2)][m.group(1)] = i
    best = []
    for blocks in loops.values():
        back = [i for i, ln in enumerate(lines) if re.match(r"\ts_c?branch\w* (\S+)", ln) and ln.split()[1] in blocks]
        region = [x.split()[0] for x in lines[min(blocks.values()):max(back) + 1] if x.startswith("\t") and x[1] not in ".;"]
        if any(o.startswith("v_mfma") for o in region) and (not best or len(region) < len(best)):
            best = region
    return collections.Counter(best)


def row(r):
    return " ".join(f"{k} {r[k]:>5}" for k, _ in FIELDS) + f" insts {r['insts']:>5}" if r else "-"


if __name__ == "__main__":
    old, new = read(sys.argv[1]), read(sys.argv[2])
    pairs = dict(a.split("=") for a in sys.argv[3:])
    names = sorted(set(new) | {n for n in old if n not in pairs})
    back = {v: k for k, v in pairs.items()}
    for n in names:
        o, w = old.get(back.get(n, n)), new.get(n)
        print(f"{n:<44} parent: {row(o):<92} result: {row(w)}")
        if o and w:
            diff = {m: (o["hist"][m], w["hist"][m]) for m in sorted(set(o["hist"]) | set(w["hist"])) if o["hist"][m] != w["hist"][m]}
            same = all(o[k] == w[k] for k in ("V", "A", "scratch", "spillV", "spillS", "LDS"))
            print(f"    resources {'EQUAL' if same else 'DIFFER'}; histogram {'EQUAL' if not diff else 'DIFFERS (parent, result): ' + str(diff)}")
            if o["loop"]:
                ldiff = {m: (o["loop"][m], w["loop"][m]) for m in sorted(set(o["loop"]) | set(w["loop"])) if o["loop"][m] != w["loop"][m]}
                print(f"    chunk loop: {sum(o['loop'].values())} / {sum(w['loop'].values())} instructions; histogram {'EQUAL' if not ldiff else 'DIFFERS (parent, result): ' + str(ldiff)}")
