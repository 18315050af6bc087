"""CPU: the one reader of the SKIMI_* environment switches (csrc/env.h) -- a stand-alone program (tests/env_probe.cpp,
host compiler, no HIP) run in child processes: defaults, atol parsing, env_once keeps its first value, env_switch keeps
it too unless SKIMI_ENV_DYNAMIC=1."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
NAME = "SKIMI_TEST_SWITCH"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path_factory.mktemp("env") / "env_probe"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", str(ROOT / "skiing_analysis_pytorch_amd" / "csrc"),
                    str(ROOT / "tests" / "env_probe.cpp"), "-o", str(exe), "-pthread"], check=True)

    def run(*args, **env):
        e = {k: v for k, v in os.environ.items() if k != NAME and k != "SKIMI_ENV_DYNAMIC"}
        e.update(env)
        out = subprocess.run([str(exe), *map(str, args)], env=e, capture_output=True, text=True, check=True).stdout
        return [int(x) for x in out.split()]

    return run


@pytest.mark.parametrize("dflt", [0, 7, -1])
def test_unset_gives_the_default(probe, dflt):
    assert probe("read", NAME, dflt) == [dflt]


@pytest.mark.parametrize("text,value", [("0", 0), ("1", 1), ("-3", -3), ("4294967296", 1 << 32), ("8589934597", (1 << 33) + 5),
                                        ("", 0), ("abc", 0), ("12abc", 12)])
@pytest.mark.parametrize("dflt", [0, 5])
def test_set_value_parses_as_atol(probe, text, value, dflt):
    """a set value wins over the default whatever it is: "0" gives 0 with a non-zero default too"""
    assert probe("read", NAME, dflt, **{NAME: text}) == [value]


def test_env_once_keeps_its_first_value(probe):
    assert probe("once", NAME, 3, 9) == [3, 3]                      # unset at the first call: the default stays
    assert probe("once", NAME, 3, 9, **{NAME: "4"}) == [4, 4]
    assert probe("once", NAME, 3, 9, SKIMI_ENV_DYNAMIC="1") == [3, 3]   # env_once does not follow SKIMI_ENV_DYNAMIC


@pytest.mark.parametrize("dynamic", [None, "0"])
def test_env_switch_keeps_its_first_value_without_dynamic(probe, dynamic):
    env = {} if dynamic is None else {"SKIMI_ENV_DYNAMIC": dynamic}
    assert probe("switch", NAME, 3, 9, **env) == [3, 3]
    assert probe("switch", NAME, 3, 9, **{NAME: "4"}, **env) == [4, 4]


def test_env_switch_follows_the_change_under_dynamic(probe):
    assert probe("switch", NAME, 3, 9, SKIMI_ENV_DYNAMIC="1") == [3, 9]
    assert probe("switch", NAME, 3, 0, **{NAME: "4"}, SKIMI_ENV_DYNAMIC="1") == [4, 0]
