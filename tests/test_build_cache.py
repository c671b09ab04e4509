"""_lib.build_library's object cache: objects are named after their whole compile command, the library after its link inputs,
and concurrent builders take turns.  A stub compiler (logs its argv, writes the -o target) keeps these fast; only the last
test runs the real hipcc."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler(path, log, then=None):
    """An executable that appends its argv to `log` and then either runs `then` with it or writes an empty -o target."""
    body = ('#!%s\nimport json, subprocess, sys\nargs = sys.argv[1:]\nwith open(%r, "a") as f:\n    f.write(json.dumps(args) + "\\n")\n'
            % (sys.executable, str(log)))
    if then:
        body += 'sys.exit(subprocess.call([%r] + args))\n' % then
    else:
        body += 'open(args[args.index("-o") + 1], "w").close()\n'
    path.write_text(body)
    path.chmod(0o755)
    return str(path)


def _calls(log):
    """(compiled source basenames, number of links) since the last call; the log is emptied."""
    lines = log.read_text().splitlines() if log.exists() else []
    log.write_text('')
    args = [json.loads(x) for x in lines]
    return sorted(os.path.basename(a[a.index('-c') + 1]) for a in args if '-c' in a), sum('-shared' in a for a in args)


@pytest.fixture()
def stub_build(tmp_path, monkeypatch):
    from pwv_amd import _lib
    log = tmp_path / 'hipcc.log'
    monkeypatch.delenv('PWV_LIB', raising=False)
    monkeypatch.delenv('PWV_CXXFLAGS', raising=False)
    monkeypatch.setenv('HIPCC', _compiler(tmp_path / 'hipcc', log))
    monkeypatch.setattr(_lib, 'LIB_PATH', str(tmp_path / 'libpwv_hip.so'))
    monkeypatch.setattr(_lib, 'OBJ_DIR', str(tmp_path / '_obj'))
    monkeypatch.setattr(_lib, 'EXTRA_FLAGS', {})
    return _lib, log


def test_an_unchanged_second_build_compiles_nothing(stub_build):
    _lib, log = stub_build
    _lib.build_library()
    assert _calls(log) == (sorted(os.path.basename(s) for s in _lib.CSRC), 1)
    _lib.build_library()
    assert _calls(log) == ([], 0)
    _lib.build_library(force=True)
    assert _calls(log) == (sorted(os.path.basename(s) for s in _lib.CSRC), 1)


def test_changed_flags_recompile_exactly_the_affected_objects(stub_build, monkeypatch, tmp_path):
    _lib, log = stub_build
    everything = sorted(os.path.basename(s) for s in _lib.CSRC)
    _lib.build_library()
    _calls(log)
    monkeypatch.setenv('PWV_CXXFLAGS', '-DPWV_TRACE')
    _lib.build_library()
    assert _calls(log) == (everything, 1)
    monkeypatch.setattr(_lib, 'EXTRA_FLAGS', {'pwv_norm.hip': ['-DX=1']})
    _lib.build_library()
    assert _calls(log) == (['pwv_norm.hip'], 1)
    # back to the first flags: its objects are still there and fresh, only the library is linked from them again
    monkeypatch.delenv('PWV_CXXFLAGS')
    monkeypatch.setattr(_lib, 'EXTRA_FLAGS', {})
    _lib.build_library()
    assert _calls(log) == ([], 1)
    _lib.build_library()
    assert _calls(log) == ([], 0)
    # another compiler is another command
    monkeypatch.setenv('HIPCC', _compiler(tmp_path / 'hipcc2', log))
    _lib.build_library()
    assert _calls(log) == (everything, 1)


def test_an_explicitly_chosen_library_is_never_rebuilt(stub_build, monkeypatch, tmp_path):
    _lib, log = stub_build
    monkeypatch.setenv('PWV_LIB', str(tmp_path / 'elsewhere.so'))
    assert _lib.build_library(force=True) == _lib.LIB_PATH
    assert _calls(log) == ([], 0) and not os.path.exists(_lib.LIB_PATH)


def test_concurrent_builds_leave_a_library_that_loads(tmp_path):
    """Two processes build the same library at once with the real hipcc (a one-function source, to stay quick): one compiles and
    links, the other waits for it and finds the result fresh, and the library loads."""
    src = tmp_path / 'mini.hip'
    src.write_text('#include <hip/hip_runtime.h>\n__global__ void mini_kernel(int* p) { p[threadIdx.x] = 1; }\n'
                   'extern "C" int pwv_version() { return 301; }\n')
    log = tmp_path / 'hipcc.log'
    lib_path = tmp_path / 'libmini.so'
    code = ('import sys; sys.path.insert(0, %r)\nfrom pwv_amd import _lib\n_lib.CSRC = [%r]\n_lib.EXTRA_FLAGS = {}\n'
            '_lib.LIB_PATH = %r\n_lib.OBJ_DIR = %r\n_lib.build_library()\n' % (ROOT, str(src), str(lib_path), str(tmp_path / '_obj')))
    env = dict(os.environ, HIPCC=_compiler(tmp_path / 'hipcc', log, then='/opt/rocm/bin/hipcc'))
    env.pop('PWV_LIB', None)
    env.pop('PWV_CXXFLAGS', None)
    procs = [subprocess.Popen([sys.executable, '-c', code], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for _ in range(2)]
    outs = [p.communicate(timeout=300)[0] for p in procs]
    assert [p.returncode for p in procs] == [0, 0], outs
    assert _calls(log) == (['mini.hip'], 1)
    assert ctypes.CDLL(str(lib_path)).pwv_version() == 301
    assert not [f for f in os.listdir(tmp_path / '_obj') if '.tmp' in f]
