"""The host rules of MI_FLAG_CHUNK_BLAKE2S -- a MemFS handle, a chunk index and the ctxs of one commit are of ONE chunk digest
algorithm, and every refusal comes before anything is walked or changed -- on the HIP test double, without a GPU
(tests/hip_stub/blake2s_scenarios.py; the digests themselves are tests/test_gpu_blake2s.py's business)."""
import os
import subprocess
import sys

from test_host_hip_double import STUB_DIR, hip_double  # noqa: F401  (the fixture builds the double when stale)


def test_handles_indexes_and_commits_keep_to_one_chunk_digest_algorithm(hip_double, tmp_path):  # noqa: F811
    env = dict(os.environ, LD_PRELOAD=(os.environ.get("LD_PRELOAD", "") + " " + hip_double).strip())
    p = subprocess.run([sys.executable, os.path.join(STUB_DIR, "blake2s_scenarios.py"), str(tmp_path)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert [ln for ln in p.stdout.splitlines() if ln.startswith("OK ")] == ["OK handle", "OK index", "OK api"]
