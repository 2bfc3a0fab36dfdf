"""The host logic of the C ABI that needs no GPU (sailfish_amd/csrc/slf_bind.h): module descriptors into module
configurations, kernel names into rows of the kernel table, argument lists into launch arguments, and the index
arithmetic of the reference's face kernels.  tests/abi_bind_main.cpp walks all of it as a stand-alone program built
with AddressSanitizer and UBSan.  Nothing is loaded into Python.  Its output must equal two records:

tests/golden/abi_binding.json: the sections resolve, bind and face, recorded from the chain of string compares and the
switches the kernel table replaced (its `config` section is the ladders' and is no longer read: the next record drops it);

tests/golden/abi_support.tsv, one line of text per case: the section `config`, the section `cross` (every feature x every
option that can offend it, malformed fields and double faults; recorded first from the refusal ladders the support table
replaced, whose codes and details it keeps) and the section `serves` (the rows of the support table, which
tests/test_serves.py compares with sailfish_amd/serves.py).

    python tests/test_abi_bind.py --record [json] [tsv]      rewrites the named records (both if none) from the present code
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)      # (run as a script, --record)
from tests import _bind  # noqa: E402
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'abi_binding.json')
SUPPORT = os.path.join(ROOT, 'tests', 'golden', 'abi_support.tsv')
JSON_SECTIONS = ('resolve', 'bind', 'face')


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
    """The program's lines: those of abi_binding.json, in its compact form, and those of abi_support.tsv, as they are."""
    lines = text.splitlines()
    return (compact('\n'.join(ln for ln in lines if ln.split('\t')[0] in JSON_SECTIONS)),
            [ln for ln in lines if ln.split('\t')[0] not in JSON_SECTIONS])


def test_binding_equals_the_recorded_behaviour(tmp_path):
    got, got_support = split(run_program(tmp_path))
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


if __name__ == '__main__':
    if sys.argv[1:2] != ['--record'] or set(sys.argv[2:]) - {'json', 'tsv'}:
        sys.exit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fix, support = split(run_program(tmp))
    if 'json' in sys.argv[2:] or not sys.argv[2:]:
        with open(FIXTURE, 'w') as fh:
            json.dump(fix, fh, separators=(',', ':'), sort_keys=True)
            fh.write('\n')
        print('%s: %d bytes' % (FIXTURE, os.path.getsize(FIXTURE)))
    if 'tsv' in sys.argv[2:] or not sys.argv[2:]:
        with open(SUPPORT, 'w') as fh:
            fh.write('\n'.join(support) + '\n')
        print('%s: %d lines, %d bytes' % (SUPPORT, len(support), os.path.getsize(SUPPORT)))
