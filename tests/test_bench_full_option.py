"""bench.py's plain run against `--full`, on CPU: bench.main() driven over a stand-in batch that records what is called on it
(tests/_bench_standin.py, one child process per command line).  A plain run makes the warm-up and timed passes and reads what
the line and --dump-outputs need, nothing else; every other leg of the benchmark runs with --full, around the same passes."""
import importlib
import json
import os
import subprocess
import sys
from unittest import mock

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 3, 2
SHAPE = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--streams", "4", "--seconds", "0.5"]
# what a plain run may call on its batch: set-up, the step, the events inside the timed region, the gate's pair for the line
PLAIN = {"Batch", "synthesize", "set_overlap", "run", "corpus_gate_enqueue", "timing_enable", "timing_read", "sync",
         "corpus_gate_read"}
DUMP = {"results", "fft", "waveform", "subblocks", "histograms"}
# what --full adds on the batch (the CPU baseline and the other configurations are switched off below: they need the oracle
# and the device)
FULL_ONLY = {"traffic_floor", "histograms", "set_true_peak_arith", "download_input", "peaks", "upload"}
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bench_standin.py"), *SHAPE, *extra],
                       capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout[-3000:]
    calls = [ln for ln in p.stderr.splitlines() if ln.startswith("CALLS ")]
    assert len(calls) == 1, p.stderr[-3000:]
    return json.loads(lines[0]), json.loads(calls[0][len("CALLS "):])


@pytest.fixture(scope="module")
def plain():
    return bench()


@pytest.fixture(scope="module")
def full():
    return bench("--full", "--no-cpu", "--no-extra")


def test_full_is_an_option_and_off_by_default():
    sys.path.insert(0, ROOT)
    try:
        with mock.patch.dict(os.environ):          # bench.py sets RCCL / HSA defaults at import: keep them out of this session
            bench_module = importlib.import_module("bench")
    finally:
        sys.path.remove(ROOT)
    ap = bench_module.arg_parser()
    assert ap.parse_args([]).full is False
    assert ap.parse_args(["--full"]).full is True


def test_plain_run_makes_its_passes_and_nothing_else(plain):
    line, calls = plain
    assert set(calls) <= PLAIN, sorted(set(calls) - PLAIN)
    assert calls.count("Batch") == 1
    assert calls.count("run") == calls.count("corpus_gate_enqueue") == STEPS + WARMUP
    assert line["full"] is False and line["steps"] == STEPS and line["warmup"] == WARMUP
    for key in HEADLINE:
        assert line[key] is not None, key
    # (the stand-in's clock: 5 ms a pass) 4 streams x 0.5 s x 48 kHz stereo per step
    assert line["ms_per_step"] == pytest.approx(5.0) and line["value"] == pytest.approx(4 * 24000 * 2 / 5e-3)
    # the legs that take runs of their own are not in a plain line
    assert line["true_peak_arithmetic"] is None and line["value_f16x3_split"] is None and line["cpu_baseline"] is None
    assert line["config"]["sustained"] is None and line["roofline"]["io_floor"] is None
    assert "pcie_inclusive_samples_per_s" not in line["config"] and "extra" not in line["config"]
    # the per-kernel events ride inside the timed steps: a plain line keeps them, over exactly those steps
    assert all(ms == 2.0 for ms in line["config"]["kernel_ms"].values()), line["config"]["kernel_ms"]


def test_plain_run_with_dump_outputs_reads_only_what_it_writes(tmp_path):
    d = str(tmp_path / "dump")
    line, calls = bench("--dump-outputs", d)
    assert set(calls) <= PLAIN | DUMP, sorted(set(calls) - PLAIN - DUMP)
    assert calls.count("run") == STEPS + WARMUP
    assert len(os.listdir(d)) == 11
    # the arrays are read behind the last timed pass
    assert max(i for i, c in enumerate(calls) if c == "run") < min(i for i, c in enumerate(calls) if c in DUMP)


def test_plain_run_in_an_overlap_mode_has_no_pass_for_kernel_times():
    line, calls = bench("--overlap", "1")
    assert set(calls) <= PLAIN and calls.count("run") == STEPS + WARMUP
    assert "timing_enable" not in calls
    assert all(ms is None for ms in line["config"]["kernel_ms"].values()) and line["config"]["sequential_gpu_ms"] is None
    assert line["ms_per_step"] is not None and line["value"] is not None


def test_full_run_keeps_every_leg_around_the_same_passes(plain, full):
    line, calls = full
    assert FULL_ONLY <= set(calls), sorted(FULL_ONLY - set(calls))
    assert line["full"] is True
    for key in HEADLINE:
        assert line[key] == plain[0][key], key
    assert line["config"]["sustained"]["steps"] >= 200 and line["roofline"]["io_floor"]["ms"] == 1.0
    assert line["true_peak_arithmetic"]["value_f16x3_split"] == line["value_f16x3_split"] is not None
    assert "pcie_inclusive_samples_per_s" in line["config"]
    # the traffic floor runs in front of the warm-up (it overwrites the spectra); everything else behind the timed steps, whose
    # calls are those of the plain run in the same order
    assert calls.index("traffic_floor") < calls.index("run")
    head = [c for c in calls[:calls.index("corpus_gate_read") + 1] if c != "traffic_floor"]
    assert head == plain[1]
    assert not FULL_ONLY & set(head)
