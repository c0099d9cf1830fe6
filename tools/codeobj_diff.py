#!/usr/bin/env python3
"""Same device code?  Compares every gfx950 kernel of two builds of libnimg.so: its disassembly (addresses and encodings
stripped, branch targets kept relative to the kernel) and its code-object metadata (register counts, LDS and scratch
sizes, spill counts, ...).  The check behind a refactor of csrc/ that must not change a kernel; no GPU needed.
    tools/codeobj_diff.py <old libnimg.so> <new libnimg.so>      prints the kernels that differ, exit status 1 if any"""
import collections, glob, os, re, shutil, subprocess, sys, tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')


def kernels(lib):
    """{kernel name: its distinct (metadata, disassembly) pairs} - several where file-local kernels of two units share a name; the
    copies every unit gets of a kernel defined in a header count once."""
    out = collections.defaultdict(list)
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, 'lib.so'))
        subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '--offloading', 'lib.so'], cwd=tmp, check=True, stdout=subprocess.DEVNULL)
        for co in sorted(glob.glob(os.path.join(tmp, 'lib.so.*gfx950*'))):
            notes = subprocess.run([os.path.join(LLVM, 'llvm-readelf'), '--notes', co], check=True, capture_output=True, text=True).stdout
            meta = {}
            for block in re.split(r'^  - (?=\.)', notes.split('amdhsa.kernels:')[-1], flags=re.M)[1:]:
                block = re.split(r'\n(?=\S)', block)[0]                           # the kernel list ends at the next top-level key
                keys = dict(re.findall(r'^(?:    )?(\.\w+): +(\S.*)$', block, flags=re.M))     # scalar keys of the kernel, not of its .args
                meta[keys['.symbol'].strip("'")[:-3]] = tuple(sorted((k, v) for k, v in keys.items() if k not in ('.name', '.symbol')))
            text = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', co], check=True, capture_output=True, text=True).stdout
            for name, body in re.findall(r'^[0-9a-f]+ <(\S+)>:\n(.*?)(?=^[0-9a-f]+ <|\Z)', text, flags=re.M | re.S):
                if name in meta:
                    body = re.sub(r'(\s|\.\.\.)+\Z', '', body)                # alignment padding behind the kernel: depends on its neighbour
                    out[name].append((meta[name], re.sub(r'// [0-9A-F]+:( [0-9A-F]{8})*', '//', body)))
    return {k: sorted(set(v)) for k, v in out.items()}


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        a, b = old.get(name), new.get(name)
        if a == b:
            continue
        bad += 1
        if a is None or b is None:
            print('%s  %s' % ('ONLY IN NEW' if a is None else 'ONLY IN OLD', name))
        elif len(a) != len(b):
            print('VARIANTS %d -> %d  %s' % (len(a), len(b), name))
        else:
            for (ma, ta), (mb, tb) in zip(a, b):
                if ma != mb:
                    print('METADATA  %s\n    old %s\n    new %s' % (name, dict(set(ma) - set(mb)), dict(set(mb) - set(ma))))
                if ta != tb:
                    print('CODE  %s  (%d -> %d lines)' % (name, ta.count('\n'), tb.count('\n')))
    print('%d kernel names in the old library, %d in the new, %d differ' % (len(old), len(new), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
