"""The environment level of a kernel switch (csrc/switches.hpp) reaches a launcher: one child process under MCEDM_WINO_SPLIT=0
launches the smallest conv the SPLIT Winograd variant serves (tests/test_hip_wino_split.py: one sample, 32 -> 32 channels, 16 x 16)
and reports the kernels the profiler named; the process-wide switch overrides the environment and gives way to it again."""
import json
import os
import subprocess
import sys

import pytest

from tests import _switches as SW

pytestmark = pytest.mark.gpu


def test_environment_level_reaches_the_launcher_and_the_process_level_overrides_it():
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, SW.__file__, "split"], env=dict(os.environ, MCEDM_WINO_SPLIT="0"),
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    names = json.loads(r.stdout.strip().splitlines()[-1])
    print(names)
    split = {k: [n for n in v if "WinoSplit" in n] for k, v in names.items()}
    assert all(names.values())                                   # every step launched something
    assert not split["env"], names
    assert split["process_on"], names
    assert not split["process_default"], names
