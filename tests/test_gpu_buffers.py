"""Who owns device memory (DevBuf in csrc/trlda_hip.hip): with every model, batch, coherence
accumulator and document index closed, the library holds no device buffer -- an exact zero, counted by
trlda_debug_device_buffers.  tests/buffers_worker.py does the work, in a process of its own: the count
is the process's, and TRLDA_MERGED_STAMPS (the buffers that once leaked) is read once per process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_closing_releases_every_device_buffer():
    from trlda_amd import _ffi
    _ffi.require_gpu()
    env = dict(os.environ, TRLDA_MERGED_STAMPS="1")
    out = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(HERE, "buffers_worker.py")],
                         env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=150)
    print(out.stdout)
    assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
    assert "buffers ok" in out.stdout
