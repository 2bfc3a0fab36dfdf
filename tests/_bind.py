"""Builds one of the stand-alone programs over the library's HIP-free host headers (tests/*_main.cpp against
sailfish_amd/csrc) with the address and undefined-behaviour sanitizers and runs it directly, as a child process: the
sanitizers' runtimes are linked into the program, nothing is preloaded and nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sailfish_amd', 'csrc')
ROCM_INCLUDE = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'include')
KNOBS = ('SLF_BC_LEVEL', 'SLF_VARIANT', 'SLF_BLOCK_X')      # the environment the headers read: the tests' own, not the caller's


def run(main_cpp, workdir, std='c++17'):
    """The finished process (returncode, stdout, stderr) of tests/<main_cpp>, built in `workdir`."""
    exe = os.path.join(str(workdir), os.path.splitext(main_cpp)[0])
    subprocess.check_call(['g++', '-std=' + std, '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           '-static-libasan', '-static-libubsan', '-Wall', '-D__HIP_PLATFORM_AMD__', '-I', ROCM_INCLUDE,
                           '-I', CSRC, '-o', exe, os.path.join(ROOT, 'tests', main_cpp)])
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    return subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


def build_and_run(main_cpp, workdir, std='c++17'):
    """The standard output of the program, which must end with status 0."""
    done = run(main_cpp, workdir, std)
    assert done.returncode == 0, '%s failed (%d):\n%s' % (main_cpp, done.returncode, done.stderr[-4000:])
    return done.stdout


def lines(main_cpp, workdir, std='c++17'):
    return [ln.split('\t') for ln in build_and_run(main_cpp, workdir, std).splitlines()]
