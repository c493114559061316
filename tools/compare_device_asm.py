"""Two outputs of `make asm` (pfemfort_amd/csrc): the same device functions with the same bodies?
usage: compare_device_asm.py before.s after.s
Bodies are compared without comments and with the compiler's local labels (.LBB<function number>_<block>) stripped of the
function number, which moves when host code instantiates templates in another order.  Exit status 1 when anything differs."""
import re
import sys


def functions(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\S+):\s*;\s*@\S+\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = re.sub(r"[ \t]*;.*$", "", m.group(2), flags=re.M)          # (comments name labels by function number too)
        out[m.group(1)] = re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", body)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    gone, new = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print(f"device functions: {len(a)} before, {len(b)} after; {len(gone)} gone, {len(new)} new, {len(differ)} bodies differ")
    for k in gone + new + differ:
        print(" ", k)
    return 1 if gone or new or differ else 0


if __name__ == "__main__":
    sys.exit(main())
