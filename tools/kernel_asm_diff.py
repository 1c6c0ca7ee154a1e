"""developer tool: compare two device assemblies of rtgo_capi.hip function by function (every kernel and every device function kept out
   of line; instruction text, comments stripped).
   hipcc <_build.HIP_FLAGS without -shared> --cuda-device-only -S -o a.s raytracingo_amd/csrc/rtgo_capi.hip    (once per tree)
   python tools/kernel_asm_diff.py a.s b.s [substring: list the differing kernels whose name contains it]"""
import re, sys


def kernels(path):
    """function symbol -> its instruction lines"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    out, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            line = line.split(";")[0].strip()
            line = re.sub(r"\.L([A-Za-z]+)\d+_(\d+)", r".L\1_\2", line)   # local labels carry the function's ordinal in the file: a new kernel shifts it
            if line and not line.startswith((".p2align", ".loc", ".file", ".cfi")):
                cur.append(line)
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
want = sys.argv[3] if len(sys.argv) > 3 else None
only = sorted(set(a) ^ set(b))
diff = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
print("functions: %d and %d; in one only: %d; identical: %d; different: %d" % (len(a), len(b), len(only), len(set(a) & set(b)) - len(diff), len(diff)))
for k in only:
    print("  only in one:", k)
for k in diff:
    if want is None or want in k:
        print("  differs: %s (%d -> %d instructions)" % (k, len(a[k]), len(b[k])))
sys.exit(1 if only or diff else 0)
