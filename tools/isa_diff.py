"""Which device functions differ between two -save-temps gfx950 assemblies (csrc/Makefile target `isa`): `python tools/isa_diff.py old.s new.s`.
A function's text = label .. .Lfunc_end with comments stripped, basic-block label numbers and its own mangled name normalised; functions are
paired by demangled name without the parameter list.  For a differing pair: the figures the compiler writes behind each function."""
import re, subprocess, sys

# the iVox kNN kernel lost its group-size and balanced-split parameters: <4, COUNT, DENSE, FIRST, true, GEN> is <COUNT, DENSE, FIRST, GEN> now
RENAMED = [(re.compile(r"ivox_knn_kernel<4, (\w+), (\w+), (\w+), true, (\w+)>"), r"ivox_knn_kernel<\1, \2, \3, \4>")]
FIELDS = [("VGPRs", r"; NumVgprs: (\d+)"), ("SGPRs", r"; TotalNumSgprs: (\d+)"), ("LDS", r"; LDSByteSize: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
          ("occupancy", r"; Occupancy: (\d+)"), ("code bytes", r"; codeLenInByte = (\d+)")]


def functions(path):
    lines = open(path).read().split("\n")
    starts = [i for i, l in enumerate(lines) if re.match(r"^_Z\w+:\s*; @", l)]
    names = subprocess.run(["c++filt"], input="\n".join(lines[i].split(":")[0] for i in starts), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for n, i in enumerate(starts):
        mangled, region = lines[i].split(":")[0], lines[i + 1:starts[n + 1] if n + 1 < len(starts) else len(lines)]
        end = next(k for k, l in enumerate(region) if l.startswith(".Lfunc_end"))
        body = []
        for l in region[:end]:
            t = l.split(";")[0].strip().replace(mangled[2:], "SELF")
            if t:
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
        tail = "\n".join(region[end:])
        stats = {"instr": sum(1 for t in body if not t.startswith(".") and not t.endswith(":"))}
        for key, pat in FIELDS:
            m = re.search(pat, tail)
            stats[key] = int(m.group(1)) if m else -1
        name, depth = names[n], 0
        for k, ch in enumerate(name):  # cut the parameter list: the first '(' outside the template arguments
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0 and k > 0 and name[k - 1] != " ":
                name = name[:k]
                break
        for pat, rep in RENAMED:
            name = pat.sub(rep, name)
        out[name] = (body, stats)
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
for side, only in (("old", sorted(set(a) - set(b))), ("new", sorted(set(b) - set(a)))):
    for name in only:
        print(f"only in {side}: {name}")
differ = [n for n in a if n in b and a[n][0] != b[n][0]]
print(f"{len(a)} / {len(b)} device functions, {len(set(a) & set(b))} paired, {len(differ)} differ")
for n in differ:
    print(n)
    for key in ["instr"] + [k for k, _ in FIELDS]:
        print(f"    {key:10s} {a[n][1][key]:7d} -> {b[n][1][key]:7d}")
