#!/usr/bin/env python3
"""Per-kernel comparison of two device-assembly files (hipcc ... -fuse-cuid=none --cuda-device-only -S).

    isa_diff.py parent.s child.s [renames.json]

A kernel is its text from `.globl sym` to `.end_amdhsa_kernel` plus its entry in the amdhsa.kernels metadata, with comments
dropped, the function index stripped from local labels and its own symbol masked.  renames.json ({"old symbol": "new symbol"}) pairs kernels whose
mangled name changed because a template parameter was dropped.  Exit status 1 if anything was added or changed."""
import hashlib, json, re, sys


def kernels(path):
    t = open(path).read()
    out = {}
    for m in re.finditer(r'\t\.globl\t(\S+)[^\n]*\n(?:(?!\t\.globl\t).)*?\.end_amdhsa_kernel', t, re.S):   # (the line may end in a comment)
        body = re.sub(r'[ \t]*;.*', '', m.group(0))      # comments: they carry function indices and are column-aligned
        body = re.sub(r'BB\d+_', 'BB_', body)            # .LBB<function index>_<block>
        body = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', body).replace(m.group(1), '@SELF@')
        out[m.group(1)] = hashlib.sha1(body.encode()).hexdigest()
    meta = t[t.index('amdhsa.kernels:'):] if 'amdhsa.kernels:' in t else ''
    for m in re.finditer(r'  - \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)', meta, re.S):
        name = re.search(r'\.name:\s+(\S+)', m.group(0)).group(1)
        out[name] = out.get(name, '') + hashlib.sha1(m.group(0).replace(name, '@SELF@').encode()).hexdigest()
    return out


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
ren = json.load(open(sys.argv[3])) if len(sys.argv) > 3 else {}
a = {ren.get(k, k): v for k, v in a.items()}
removed, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
changed = sorted(k for k in a if k in b and a[k] != b[k])
print(f'{sys.argv[1]}: {len(a)} kernels, {sys.argv[2]}: {len(b)}')
for tag, names in (('removed', removed), ('added', added), ('changed', changed)):
    for n in names:
        print(f'  {tag}: {n}')
sys.exit(1 if added or changed else 0)
