"""Compare two `make asm` listings function by function, whatever the order of the functions in them:
`python cmpasm.py parent/pfem_device.gfx950.s pfem_device.gfx950.s` exits 0 when both hold the same symbols with the same bodies."""
import collections, re, sys


def split(path):
    funcs, rest, name, buf = {}, [], None, []
    for line in open(path):
        m = re.search(r'; -- Begin function (\S+)', line)
        if m:
            name, buf = m.group(1), []
        if name is None:
            rest.append(line)
            continue
        # local labels, and the comments that quote them, carry the function's ordinal in the file
        line = re.sub(r'\.(LBB|LJTI|Lfunc_begin|Lfunc_end)\d+', r'.\1#', line)
        buf.append(re.sub(r'(Header=|Loop )BB\d+_', r'\1BB#_', line))
        if '; -- End function' in line:
            assert name not in funcs, name
            funcs[name], name = ''.join(buf), None
    return funcs, collections.Counter(rest)


(a, ra), (b, rb) = split(sys.argv[1]), split(sys.argv[2])
differ = sorted(k for k in a.keys() & b.keys() if a[k] != b[k])
print("%d / %d functions; only in the first %d, only in the second %d, bodies that differ %d; lines outside functions %s" % (
    len(a), len(b), len(a.keys() - b.keys()), len(b.keys() - a.keys()), len(differ), "equal" if ra == rb else "DIFFER"))
for k in sorted(a.keys() ^ b.keys()) + differ:
    print("  ", k)
sys.exit(0 if a.keys() == b.keys() and not differ and ra == rb else 1)
