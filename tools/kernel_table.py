#!/usr/bin/env python3
"""Per-kernel resource table of every HIP source of a tree, and the comparison of two such tables.

    python tools/kernel_table.py table [ROOT [ASMDIR]] > table.txt   # compile ROOT's csrc/*.hip device-only
    python tools/kernel_table.py diff parent.txt new.txt [--pair OLD=NEW:ARG ...]
    python tools/kernel_table.py summary table.txt > summary.txt     # one line per kernel template

A table line is, per kernel symbol, sorted by demangled name:

    vgpr agpr sgpr scratch lds occupancy codeLenInByte body-hash  demangled name

Sources are compiled with ``_build.py``'s FLAGS and FILE_FLAGS.  ``body-hash`` is the SHA-1 of the
instruction text between the kernel's entry label and its ``.Lfunc_end``, basic-block labels
renumbered in order of appearance, so two tables agree on a kernel exactly when its code does.

``diff --pair OLD=NEW:ARG ...`` pairs every old kernel ``OLD<A...>`` with ``NEW<A..., ARG>``, for any
number of such mappings: ``encode_generic_kernel=codec_generic_kernel:false
decode_generic_kernel=codec_generic_kernel:true`` for two kernels merged on a trailing ``bool``.  A
pair must keep vgpr, agpr, scratch, lds and occupancy; sgpr and code length may move with the kernel
argument layout and are reported when they do, as is a body hash that differs.

A full table has a line per instantiation (some 1500 of them); ``summary`` condenses one to a line
per kernel template: the number of instantiations, the range of each number over them, and a digest
of their table lines, so two summaries agree on a template exactly when the full tables do.
"""
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CXXFILT = 'c++filt'
INFO = [('vgpr', r'; NumVgprs: (\d+)'), ('agpr', r'; NumAgprs: (\d+)'), ('sgpr', r'; TotalNumSgprs: (\d+)'),
        ('scratch', r'; ScratchSize: (\d+)'), ('lds', r'; LDSByteSize: (\d+)'), ('occ', r'; Occupancy: (\d+)'),
        ('len', r'; codeLenInByte = (\d+)')]


def _body_hash(body):
    labels = {}
    def renum(m):
        return labels.setdefault(m.group(0), f'.L{len(labels)}')
    lines = [ln.split(';')[0].rstrip() for ln in body.split('\n')]
    text = '\n'.join(ln for ln in lines if ln.strip())
    return hashlib.sha1(re.sub(r'\.L[A-Za-z_]*\d+(_\d+)?', renum, text).encode()).hexdigest()[:12]


def kernels_of(asm):
    """{mangled name: (numbers..., body hash)} of one device assembly file"""
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', asm, re.M))
    out = {}
    for m in re.finditer(r'^(\S+):\s*;\s*@\S+\n', asm, re.M):
        name = m.group(1)
        if name not in kernels:
            continue
        end = asm.index('.Lfunc_end', m.end())
        body = asm[m.end():end].split('.amdhsa_kernel')[0]  # the kernel descriptor sits before .Lfunc_end
        out[name] = tuple(int(re.compile(pat).search(asm, end).group(1)) for _, pat in INFO) + (_body_hash(body),)
    return out


def table(root, keep=None):
    spec = importlib.util.spec_from_file_location('_build', os.path.join(root, 'kompressor_amd', '_build.py'))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    rows = {}
    with tempfile.TemporaryDirectory() as tmp:
        d = keep or tmp  # ASMDIR: keep the assembly files
        os.makedirs(d, exist_ok=True)

        def one(src):
            s = os.path.join(d, os.path.basename(src) + '.s')
            if not (os.path.exists(s) and os.path.getmtime(s) >= b._headers_mtime() and
                    os.path.getmtime(s) >= os.path.getmtime(src)):  # a kept file of this source as it is
                subprocess.run([b.HIPCC, *b.FLAGS, *b.FILE_FLAGS.get(os.path.basename(src), []), '--cuda-device-only',
                                '-S', src, '-o', s], check=True)
            return kernels_of(open(s).read())
        with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
            for ks in ex.map(one, b.sources()):
                rows.update(ks)
    names = subprocess.run([CXXFILT], input='\n'.join(rows), capture_output=True, text=True, check=True).stdout.split('\n')
    print('# ' + ' '.join(k for k, _ in INFO) + ' body-hash  kernel')
    for dem, mangled in sorted(zip(names, rows)):
        print(' '.join(str(v) for v in rows[mangled]) + '  ' + dem)


def read_table(path):
    out = {}
    for ln in open(path):
        if ln.startswith('#') or not ln.strip():
            continue
        nums, name = ln.rstrip('\n').split('  ', 1)
        out[name] = nums.split(' ')
    return out


PAIR_KEEPS = [i for i, (k, _) in enumerate(INFO) if k in ('vgpr', 'agpr', 'scratch', 'lds', 'occ')]


def diff(a_path, b_path, pairs):
    a, b = read_table(a_path), read_table(b_path)
    bad = 0
    mapping = {old: new.rsplit(':', 1) for old, new in (p.split('=', 1) for p in pairs)}
    if mapping:
        renamed = {}
        for name, row in a.items():
            m = re.match(r'(void kmp::)(%s)<(.*)>\(' % '|'.join(map(re.escape, mapping)), name)
            if not m:
                renamed[name] = row
                continue
            new, arg = mapping[m.group(2)]
            want = f'{m.group(1)}{new}<{m.group(3)}, {arg}>('
            got = [n for n in b if n.startswith(want)]
            if len(got) != 1:
                print(f'UNPAIRED {name}')
                bad += 1
                continue
            nb = b.pop(got[0])
            if [nb[i] for i in PAIR_KEEPS] != [row[i] for i in PAIR_KEEPS]:
                print(f'NUMBERS DIFFER {name}\n  parent {row}\n  new    {nb}')
                bad += 1
            elif nb != row:
                moved = ', '.join(f'{k} {row[i]} -> {nb[i]}' for i, (k, _) in enumerate(INFO) if nb[i] != row[i])
                print(f'paired, {moved or "numbers equal"}, text differs: {name}\n    -> {got[0]}')
            else:
                print(f'paired, identical code: {name}\n    -> {got[0]}')
        a = renamed
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f'ONLY IN {"parent" if name in a else "new"}: {name}')
            bad += 1
        elif a[name] != b[name]:
            print(f'DIFFERS {name}\n  parent {a[name]}\n  new    {b[name]}')
            bad += 1
    print(f'{len(a)} kernels compared by name, {bad} mismatches')
    return 1 if bad else 0


def summary(path):
    groups = {}
    for name, row in read_table(path).items():
        groups.setdefault(name.split('<')[0].split('(')[0], []).append((row, name))
    print('# count ' + ' '.join(k for k, _ in INFO) + ' (min..max) digest  kernel template')
    for key, rows in sorted(groups.items()):
        cols = [sorted(int(r[i]) for r, _ in rows) for i in range(len(INFO))]
        rng = ' '.join(str(c[0]) if c[0] == c[-1] else f'{c[0]}..{c[-1]}' for c in cols)
        digest = hashlib.sha1('\n'.join(sorted(' '.join(r) + '  ' + n for r, n in rows)).encode()).hexdigest()[:12]
        print(f'{len(rows)} {rng} {digest}  {key}')


if __name__ == '__main__':
    if sys.argv[1] == 'table':
        table(os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else
              os.path.dirname(os.path.dirname(os.path.abspath(__file__))), sys.argv[3] if len(sys.argv) > 3 else None)
    elif sys.argv[1] == 'summary':
        summary(sys.argv[2])
    else:
        sys.exit(diff(sys.argv[2], sys.argv[3], sys.argv[sys.argv.index('--pair') + 1:] if '--pair' in sys.argv else []))
