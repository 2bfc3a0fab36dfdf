"""The host logic of the C ABI that needs no GPU (sailfish_amd/csrc/slf_bind.h): module descriptors into module
configurations, kernel names into rows of the kernel table, argument lists into launch arguments, and the index
arithmetic of the reference's face kernels.  tests/abi_bind_main.cpp walks all of it as a stand-alone program built
with AddressSanitizer and UBSan; its output must equal tests/golden/abi_binding.json, recorded from the chain of
string compares and the switches this table replaced.  Nothing is loaded into Python.

    python tests/test_abi_bind.py --record      rewrites the fixture from the present code
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')
MAIN = os.path.join(ROOT, 'tests', 'abi_bind_main.cpp')
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'abi_binding.json')
ROCM_INCLUDE = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include')


def run_program(workdir):
    exe = os.path.join(str(workdir), 'abi_bind')
    # the sanitizers' runtimes are linked into the program: it does not depend on what else the process environment loads
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-static-libasan', '-static-libubsan', '-Wall', '-D__HIP_PLATFORM_AMD__', '-I', ROCM_INCLUDE,
                           '-I', CSRC, '-o', exe, MAIN])
    env = {k: v for k, v in os.environ.items() if k not in ('SLF_BC_LEVEL', 'SLF_VARIANT', 'SLF_BLOCK_X')}
    done = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert done.returncode == 0, 'abi_bind_main failed (%d):\n%s' % (done.returncode, done.stderr[-4000:])
    return done.stdout


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


def test_binding_equals_the_recorded_behaviour(tmp_path):
    got = compact(run_program(tmp_path))
    want = json.load(open(FIXTURE))
    if got != want:
        g, w = expand(got), expand(want)
        assert sorted(g) == sorted(w), ('cases differ', sorted(set(g) ^ set(w))[:10])
        wrong = [(k, g[k], w[k]) for k in sorted(w) if g[k] != w[k]]
        assert not wrong, ('%d cases differ; (case, got, recorded):' % len(wrong), wrong[:5])
    assert got == want
    # the matrix is the one the fixture was recorded for: nothing fell out of it unnoticed
    w = expand(want)
    sections = {s: sum(1 for k in w if k[0] == s) for s in ('config', 'resolve', 'bind', 'face')}
    assert sections['config'] >= 48 + 40 and sections['resolve'] >= 1500 and sections['bind'] >= 6000 and sections['face'] >= 100, sections
    refusals = set(m for (s, _, _, _), (code, m, _) in w.items() if s == 'config' and code)
    assert len(refusals) >= 40, len(refusals)
    assert not any(k[3] == 'no-signature' for k in w)


if __name__ == '__main__':
    if sys.argv[1:] != ['--record']:
        sys.exit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fix = compact(run_program(tmp))
    with open(FIXTURE, 'w') as fh:
        json.dump(fix, fh, separators=(',', ':'), sort_keys=True)
        fh.write('\n')
    print('%s: %d bytes' % (FIXTURE, os.path.getsize(FIXTURE)))
