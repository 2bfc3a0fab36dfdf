#!/usr/bin/env python3
"""Is the device code of two trees of this repository the same?

usage: device_code_diff.py PARENT_TREE THIS_TREE [--jobs N] [--asm-dir DIR]

Every source of sailfish_amd/build.py SOURCES is compiled to gfx950 assembly in both trees, with the flags that tree's
build.py names (device side only, -S), and the listings are compared function by function.  Inside a function its own
mangled symbol is replaced by a placeholder, and the __hip_cuid_* symbol of the translation unit everywhere, so that a
kernel whose template arguments are spelled differently but whose code is the same compares equal.  One line per object:

  <object> identical functions N                      the listings are the same text, symbol names included
  <object> functions A -> B bodies <how> descriptors <how> metadata <how>
      bodies       in-order: the same sequence of function bodies | reordered: the same multiset | DIFFER
      descriptors  in-order: the .amdhsa_* blocks (VGPRs, SGPRs, scratch, LDS ...) are the same sequence | DIFFER
      metadata     same: what follows the last function (kernel arguments, resources), symbols replaced by their position
                   | DIFFER

Exit status 1 if any object has a DIFFER.  --asm-dir keeps the listings (DIR/parent, DIR/this) and reuses one that is
newer than every file under the tree's csrc/.  Hashes and compares text, nothing else.
"""
import argparse
import collections
import concurrent.futures
import hashlib
import os
import re
import runpy
import subprocess
import sys
import tempfile

BEGIN = re.compile(r'; -- Begin function (\S+)')
CUID = re.compile(r'__hip_cuid_[0-9a-f]+')


def tree_build(tree):
    b = runpy.run_path(os.path.join(tree, 'sailfish_amd', 'build.py'), run_name='build_of_tree')
    flags = [f for f in b['HIPCC_FLAGS'] if f != '-shared']
    return b['_hipcc'](), flags, b['SOURCES'], os.path.join(tree, 'sailfish_amd', 'csrc')


def compile_listing(hipcc, flags, csrc, src, out):
    newest = max(os.path.getmtime(os.path.join(csrc, f)) for f in os.listdir(csrc))
    if os.path.exists(out) and os.path.getmtime(out) > newest:
        return out
    subprocess.check_call([hipcc] + flags + ['--cuda-device-only', '-S', '-o', out, src], cwd=csrc, stderr=subprocess.DEVNULL)
    return out


def split(text):
    """-> (what precedes the first function, [(symbol, text)], what follows the last one)"""
    lines = text.split('\n')
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [BEGIN.search(ln)] if m]
    if not starts:
        return text, [], ''
    # the .section / .text line in front of a "Begin function" line belongs to that function
    first = [i - 1 if i > 0 and re.match(r'\s*\.(section|text)\b', lines[i - 1]) else i for i, _ in starts]
    end = len(lines)
    for i in range(starts[-1][0], len(lines)):
        if lines[i].startswith('\t.section\t.AMDGPU.gpr_maximums') or lines[i].startswith('\t.amdgpu_metadata'):
            end = i
            break
    funcs = []
    for k, (_, name) in enumerate(starts):
        stop = first[k + 1] if k + 1 < len(starts) else end
        funcs.append((name, '\n'.join(lines[first[k]:stop])))
    return '\n'.join(lines[:first[0]]), funcs, '\n'.join(lines[end:])


def digest(s):
    return hashlib.sha256(s.encode()).hexdigest()


def summarise(path):
    text = CUID.sub('__hip_cuid_X', open(path, errors='replace').read())
    head, funcs, tail = split(text)
    bodies, descs = [], []
    for name, body in funcs:
        body = body.replace(name, '<SELF>')
        bodies.append(digest(body))
        descs.append(digest('\n'.join(ln for ln in body.split('\n') if ln.lstrip().startswith('.amdhsa_'))))
    # longest names first: a symbol may be the prefix of another
    order = sorted(range(len(funcs)), key=lambda k: -len(funcs[k][0]))
    for k in order:
        tail = tail.replace(funcs[k][0], '<F%d>' % k)
    return {'whole': digest(text), 'n': len(funcs), 'bodies': bodies, 'descs': descs, 'rest': digest(head + '\0' + tail)}


def compare(name, a, b):
    if a['whole'] == b['whole']:
        return True, '%s identical functions %d' % (name, a['n'])
    if a['bodies'] == b['bodies']:
        bodies = 'in-order'
    elif collections.Counter(a['bodies']) == collections.Counter(b['bodies']):
        bodies = 'reordered'
    else:
        bodies = 'DIFFER'
    descs = 'in-order' if a['descs'] == b['descs'] else 'DIFFER'
    rest = 'same' if a['rest'] == b['rest'] else 'DIFFER'
    ok = a['n'] == b['n'] and 'DIFFER' not in (bodies, descs, rest)
    return ok, '%s functions %d -> %d bodies %s descriptors %s metadata %s' % (name, a['n'], b['n'], bodies, descs, rest)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('parent_tree')
    ap.add_argument('this_tree')
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument('--asm-dir')
    args = ap.parse_args()
    jobs = max(1, min(16, args.jobs))
    tmp = None if args.asm_dir else tempfile.TemporaryDirectory()
    root = args.asm_dir or tmp.name
    trees = {'parent': tree_build(args.parent_tree), 'this': tree_build(args.this_tree)}
    sources = trees['this'][2]
    missing = [s for s in sources if s not in trees['parent'][2]]
    if missing:
        sys.exit('not in the parent tree: ' + ' '.join(missing))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        futures = {}
        for side, (hipcc, flags, _, csrc) in trees.items():
            os.makedirs(os.path.join(root, side), exist_ok=True)
            for src in sources:
                out = os.path.join(root, side, src.replace('.hip', '.s'))
                futures[side, src] = pool.submit(compile_listing, hipcc, flags, csrc, src, out)
        all_ok = True
        for src in sources:
            a, b = (summarise(futures[side, src].result()) for side in ('parent', 'this'))
            ok, line = compare(src.replace('.hip', ''), a, b)
            all_ok = all_ok and ok
            print(line, flush=True)
    return 0 if all_ok else 1


if __name__ == '__main__':
    sys.exit(main())
