"""The host logic of the C ABI that needs no GPU (sailfish_amd/csrc/slf_bind.h): module descriptors into module
configurations, kernel names into rows of the kernel table, argument lists into launch arguments, and the index
arithmetic of the reference's face kernels.  tests/abi_bind_main.cpp walks all of it as a stand-alone program built
with AddressSanitizer and UBSan.  Nothing is loaded into Python.  Its output must equal three records:

tests/golden/abi_binding.json: the sections resolve, bind and face, recorded from the chain of string compares and the
switches the kernel table replaced (its `config` section is the ladders' and is no longer read: the next record drops it);

tests/golden/abi_support.tsv, one line of text per case: the section `config`, the section `cross` (every feature x every
option that can offend it, malformed fields and double faults; recorded first from the refusal ladders the support table
replaced, whose codes and details it keeps) and the section `serves` (the rows of the support table, which
tests/test_serves.py compares with sailfish_amd/serves.py);

tests/golden/abi_launch.tsv, one line of text per case: what a launch refuses and with which step and rows it runs (section
`launch`: every kernel kind in the modules that serve it, regions at each edge of the real nodes, the iteration of AA
kernels, NULL maps and node tables, the acceleration field, an armed pair sweep, the direction limit of the box kinds, and
double faults that pin the order of the checks) and the argument checks of CollideAndPropagateResident and of the x-face
setters (sections `resident`, `xface-buffers`, `xface-planes`).  Recorded from the code of slf_kernel_launch and of the
setters that part (f) of slf_bind.h replaced.  These refusals are what stands between a caller and an out-of-bounds kernel:
they are tested here and not on a GPU, where a test against a broken check would be a wild store.

    python tests/test_abi_bind.py --record [json] [tsv] [launch]      rewrites the named records (all if none) from the present code
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)      # (run as a script, --record)
from tests import _bind  # noqa: E402
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'abi_binding.json')
SUPPORT = os.path.join(ROOT, 'tests', 'golden', 'abi_support.tsv')
LAUNCH = os.path.join(ROOT, 'tests', 'golden', 'abi_launch.tsv')
JSON_SECTIONS = ('resolve', 'bind', 'face')
LAUNCH_SECTIONS = ('launch', 'resident', 'xface-buffers', 'xface-planes')


def run_program(workdir):
    return _bind.build_and_run('abi_bind_main.cpp', workdir)


def compact(text):
    """The program's lines as the fixture stores them: every message and every detail string once, the configurations
    by number, and the configurations that give the same answer to (section, subject, try) in one entry."""
    messages, details, configs, cases = [], [], [], {}

    def index(table, s):
        if s not in table:
            table.append(s)
        return table.index(s)

    lookup = {}
    for ln in text.splitlines():
        section, subject, config, what, code, message, detail = ln.split('\t')
        cfg = index(configs, config)
        answer = (int(code), index(messages, message), index(details, detail))
        groups = cases.setdefault(section, {}).setdefault(subject, {}).setdefault(what, [])
        key = (section, subject, what, answer)
        if key not in lookup:
            lookup[key] = [answer[0], answer[1], answer[2], []]
            groups.append(lookup[key])
        lookup[key][3].append(cfg)
    return {'messages': messages, 'details': details, 'configs': configs, 'cases': cases}


def expand(fix):
    """{(section, subject, configuration, try): (code, message, detail)}"""
    out = {}
    for section, subjects in fix['cases'].items():
        for subject, tries in subjects.items():
            for what, groups in tries.items():
                for code, mi, di, cfgs in groups:
                    for c in cfgs:
                        out[(section, subject, fix['configs'][c], what)] = (code, fix['messages'][mi], fix['details'][di])
    return out


def split(text):
    """The program's lines: those of abi_binding.json, in its compact form, and those of abi_support.tsv and of
    abi_launch.tsv, as they are."""
    lines = text.splitlines()
    return (compact('\n'.join(ln for ln in lines if ln.split('\t')[0] in JSON_SECTIONS)),
            [ln for ln in lines if ln.split('\t')[0] not in JSON_SECTIONS + LAUNCH_SECTIONS],
            [ln for ln in lines if ln.split('\t')[0] in LAUNCH_SECTIONS])


def test_binding_equals_the_recorded_behaviour(tmp_path):
    got, got_support, got_launch = split(run_program(tmp_path))
    want = json.load(open(FIXTURE))
    want['cases'] = {s: want['cases'][s] for s in JSON_SECTIONS}
    g, w = expand(got), expand(want)
    assert sorted(g) == sorted(w), ('cases differ', sorted(set(g) ^ set(w))[:10])
    wrong = [(k, g[k], w[k]) for k in sorted(w) if g[k] != w[k]]
    assert not wrong, ('%d cases differ; (case, got, recorded):' % len(wrong), wrong[:5])
    want_support = open(SUPPORT).read().splitlines()
    assert len(got_support) == len(want_support), (len(got_support), len(want_support))
    wrong = [(a, b) for a, b in zip(got_support, want_support) if a != b]
    assert not wrong, ('%d lines differ; (got, recorded):' % len(wrong), wrong[:5])
    # the matrix is the one the records were made for: nothing fell out of it unnoticed
    sections = {s: sum(1 for k in w if k[0] == s) for s in JSON_SECTIONS}
    sections.update({s: sum(1 for ln in want_support if ln.startswith(s + '\t')) for s in ('config', 'cross', 'serves')})
    assert sections['config'] >= 48 + 40 and sections['resolve'] >= 1500 and sections['bind'] >= 6000 and sections['face'] >= 100, sections
    assert sections['cross'] >= 16 * 39 + 20 and sections['serves'] >= 11, sections
    refusals = set(ln.split('\t')[5] for ln in want_support if ln.startswith('config\t') and ln.split('\t')[4] != '0')
    assert len(refusals) >= 40, len(refusals)
    assert not any(k[3] == 'no-signature' for k in w)
    want_launch = open(LAUNCH).read().splitlines()
    assert len(got_launch) == len(want_launch), (len(got_launch), len(want_launch))
    wrong = [(a, b) for a, b in zip(got_launch, want_launch) if a != b]
    assert not wrong, ('%d lines differ; (got, recorded):' % len(wrong), wrong[:5])
    # ... and every refusal of part (f) is in the record, each kernel kind of the table among the launches
    cases = [ln.split('\t') for ln in want_launch]
    sections.update({s: sum(1 for c in cases if c[0] == s) for s in LAUNCH_SECTIONS})
    refusals = {s: set(c[5] for c in cases if c[0] == s and c[4] != '0') for s in LAUNCH_SECTIONS}
    assert len(refusals['launch']) >= 11 and len(refusals['resident']) >= 8, refusals
    assert len(refusals['xface-buffers']) >= 6 and len(refusals['xface-planes']) >= 9, refusals
    launched = set(c[1] for c in cases if c[0] == 'launch' and c[3] == 'no-region' and c[4] == '0')
    table = set(r[1] for r in (k for k in w if k[0] == 'resolve') if r[1] not in ('', 'NoSuchKernel', 'CollideAndPropagateResident'))
    assert launched == table, launched ^ table


if __name__ == '__main__':
    if sys.argv[1:2] != ['--record'] or set(sys.argv[2:]) - {'json', 'tsv', 'launch'}:
        sys.exit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fix, support, launch = split(run_program(tmp))
    if 'json' in sys.argv[2:] or not sys.argv[2:]:
        with open(FIXTURE, 'w') as fh:
            json.dump(fix, fh, separators=(',', ':'), sort_keys=True)
            fh.write('\n')
        print('%s: %d bytes' % (FIXTURE, os.path.getsize(FIXTURE)))
    if 'tsv' in sys.argv[2:] or not sys.argv[2:]:
        with open(SUPPORT, 'w') as fh:
            fh.write('\n'.join(support) + '\n')
        print('%s: %d lines, %d bytes' % (SUPPORT, len(support), os.path.getsize(SUPPORT)))
    if 'launch' in sys.argv[2:] or not sys.argv[2:]:
        with open(LAUNCH, 'w') as fh:
            fh.write('\n'.join(launch) + '\n')
        print('%s: %d lines, %d bytes' % (LAUNCH, len(launch), os.path.getsize(LAUNCH)))
