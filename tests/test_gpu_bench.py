"""GPU: a plain ``bench.py`` run (no ``--full``) on a small C2-shaped workload: it times exactly
``--steps`` steps, runs none of the legs that ``--full`` adds, and ``--dump-outputs`` writes the last
timed step's outputs, identical from run to run (the inputs depend on the arguments alone)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CERTS, VOTES = 400, 67   # 26,800 signatures: above the latency-mode launch size, several workgroups
FULL_ONLY = ("host_fed", "msm", "worker_digest", "latency", "digest", "c4")


def _plain_run(capsys, out_dir):
    import bench
    assert bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1", "--certs", str(CERTS),
                       "--key-window", "13",   # small key tables: set-up well under a second
                       "--dump-outputs", str(out_dir)]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {n[:-4]: np.load(os.path.join(out_dir, n)) for n in sorted(os.listdir(out_dir))}


def test_plain_run_dumps_the_last_step_and_repeats(capsys, tmp_path):
    d, a = _plain_run(capsys, tmp_path / "a")
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1
    assert d["checks"]["ok"] and d["checks"]["timed_steps_checked"] == 3 and d["checks"]["steps_checked"] == 4
    assert d["unit"] == "sigs/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(3 * CERTS * VOTES / (3 * d["ms_per_step"] / 1e3))
    assert not any(k in d for k in FULL_ONLY) and d["cpu_baseline"] is None
    assert d["roofline"]["isolated"] is None and d["p50_cert_latency_ms"] is None
    assert sorted(a) == ["cert_ok", "sig_flags", "stake", "status"]
    assert a["cert_ok"].dtype == np.float32 and a["cert_ok"].shape == (CERTS,) and (a["cert_ok"] == 1).all()
    assert a["stake"].dtype == np.float64 and (a["stake"] == VOTES).all()
    assert a["status"].dtype == np.float32 and a["status"].tolist() == [0.0]
    assert a["sig_flags"].dtype == np.float32 and a["sig_flags"].shape == (CERTS * VOTES,)
    assert (a["sig_flags"].astype(np.int64) & 0x008 != 0).all()   # NW_F_STRICT on every honest vote
    assert d["outputs_dumped"] == {k: list(v.shape) for k, v in a.items()}
    _, b = _plain_run(capsys, tmp_path / "b")
    assert sorted(b) == sorted(a) and all(np.array_equal(a[k], b[k]) for k in a)
