#!/usr/bin/env python3
"""Has the device code moved?  Compares two builds' device assembly function by function (mangled symbol).

    make -C lightcurve_fitting_amd/csrc asm                      # the product build's lcf_*.s, here and in the other tree
    python tools/isa_diff.py --old <old tree>/csrc/*.s --new lightcurve_fitting_amd/csrc/lcf_*.s [-v]

A function is its instruction text, its .amdhsa_* kernel descriptor and its resource symbols (.set <name>.num_vgpr ...),
comments dropped and local labels renumbered (.LBB<function>_<n>: the function index changes when a kernel changes
file).  Both sides must hold the same functions, each once -- a kernel compiled into two files is reported.  Exit status
0 only if nothing is missing, new, twice or different.
"""
import argparse
import collections
import difflib
import re
import sys


def functions(paths):
    """{symbol: [normalised text, one per definition]} of the assembly files."""
    out = collections.defaultdict(list)
    for path in paths:
        name, body = None, []
        for line in open(path):
            m = re.match(r'\s*\.type\s+(\S+),@function', line)
            if m or line.startswith('\t.section\t.AMDGPU.csdata'):
                if name:
                    out[name].append(body)
                name, body = (m.group(1), []) if m else (None, [])
                continue
            line = re.sub(r'(\.L[A-Za-z_]+?)\d+(_\d+)?\b', r'\1\2', line.split(';')[0]).strip()
            if name and line:
                body.append(line)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--old', nargs='+', required=True)
    ap.add_argument('--new', nargs='+', required=True)
    ap.add_argument('-v', action='store_true', help='print the diff of every function that differs')
    args = ap.parse_args()
    old, new = functions(args.old), functions(args.new)
    missing, added = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    twice = sorted(f for side in (old, new) for f, defs in side.items() if len(defs) > 1)
    common = sorted(set(old) & set(new))
    different = [f for f in common if old[f][0] != new[f][0]]
    for what, names in (('missing', missing), ('new', added), ('twice', twice), ('different', different)):
        for f in names:
            print(f'{what}: {f}')
    if args.v:
        for f in different:
            sys.stdout.writelines(l + '\n' for l in difflib.unified_diff(old[f][0], new[f][0], 'old ' + f, 'new ' + f, lineterm=''))
    print(f'isa_diff: {len(common)} functions compared, {len(common) - len(different)} identical, {len(different)} different; '
          f'{len(missing)} missing, {len(added)} new, {len(twice)} twice')
    return 1 if missing or added or twice or different else 0


if __name__ == '__main__':
    sys.exit(main())
