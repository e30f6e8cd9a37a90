"""Cross-stream ordering under the library's own queue count (EXPERIMENTS.md O.1 - O.3).

tests/stream_order_cases.py runs ONCE, as a fresh child process with GPU_MAX_HW_QUEUES=16 - what the library sets for
itself (csrc/api.hip) and what this suite's own process, started with another value, never runs under: with fewer
hardware queues most stream pairs share a queue and run in order whatever the library's waits say.  The child delays a
producer's (or a consumer's) stream with vmpc_ctx_debug_delay, calls the library, compares with the oracle, and records
for every Context.wait_for whether the producer's stream was still busy.  The tests here only read the records; a child
that fails or runs out of time fails every one of them, and nothing is retried."""
import json
import os
import subprocess
import sys

import pytest

from tests import stream_order_cases as soc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 300


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    out_path = tmp_path_factory.mktemp("stream_order") / "records.json"
    env = dict(os.environ, GPU_MAX_HW_QUEUES=soc.QUEUES)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_order_cases.py"), "--out", str(out_path)],
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT_S, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-3000:], out.stderr[-3000:])
    with open(out_path) as f:
        doc = json.load(f)
    assert doc["queues"] == soc.QUEUES
    print(f"stream order child: {len(doc['records'])} cases in {doc['wall_s']} s")
    return {r["case"]: r for r in doc["records"]}


def test_every_case_ran(records):
    assert sorted(records) == sorted(soc.CASE_NAMES)


@pytest.mark.parametrize("pair", soc.CANARY_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_pair_is_concurrent_under_the_library_queue_count(records, pair):
    """without a wait the second stream's copy reads the OLD bytes (the pair really overlaps: a missing wait in a case
    over it would show), with the wait the new ones"""
    rec = records[f"canary_{pair[0]}_{pair[1]}"]
    assert rec["ok"], rec["error"]
    assert rec["no_wait"] == "old" and rec["with_wait"] == "new"


@pytest.mark.parametrize("name", [n for n, kind, _ in soc.CASES if kind == "hook"])
def test_delay_hook(records, name):
    rec = records[name]
    assert rec["ok"], rec["error"]
    if name == "hook_timing":
        assert rec["requested_us"] / 1000.0 <= rec["measured_ms"] <= rec["upper_ms"]


@pytest.mark.parametrize("name", [n for n, kind, _ in soc.CASES if kind == "raw"])
def test_read_after_write(records, name):
    """the producer's stream delayed: the result is the oracle's, and the row's wait_for saw the producer still busy
    (host_us: the host time from the stall to that wait; the delays were chosen as at least twice what was measured)"""
    rec = records[name]
    assert not rec["blind"], rec["error"]
    assert rec["ok"], rec["error"]
    assert rec["host_us"] is not None, rec
    assert any(not w["done"] for w in rec["waits"])


@pytest.mark.parametrize("name", [n for n, kind, _ in soc.CASES if kind == "war"])
def test_write_after_read(records, name):
    """the consumer's stream delayed, the caller goes on with the same buffers: both results are the oracle's"""
    rec = records[name]
    assert rec["ok"], rec["error"]
    assert rec["waits"]


@pytest.mark.parametrize("name", [n for n, kind, _ in soc.CASES if kind == "native"])
def test_native_event_orderings(records, name):
    """ev_sorted / ev_bucketed around a shared bucket stream, the landed counts of the chunked text copies: the call
    returned with its work still queued behind the delay, and the result is the oracle's"""
    rec = records[name]
    assert rec["ok"], rec["error"]
    assert rec["pending_when_enqueued"]
