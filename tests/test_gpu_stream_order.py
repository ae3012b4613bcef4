"""Every native entry point on a non-blocking side stream behind pending work (the protocol, the delay and the cases:
tests/stream_checks.py).  Each case must give, bit for bit, what the same call gives on the default stream, although its inputs
were copied into place on the side stream behind a 100 ms delay kernel and every workspace held another problem's values; and,
unless the entry is documented to block the host (stream_checks.HOST_SYNCHRONISING, INTEGRATION.md "Streams"), the call must
have returned while the stream was still blocked.  The suite cannot see a wrong-stream launch that happens to share a hardware
queue with the sleeping stream; that can hide a bug, never produce a false failure.  Run with ``-m gpu``.

Measured on an MI355X: profiles/stream_order.txt (tools/stream_order.py).
"""
import pytest

import stream_checks as sc

pytestmark = pytest.mark.gpu


def test_harness_detects_a_wrong_stream_op():
    """The positive control: an op deliberately issued on the default stream while the side stream sleeps.  The default stream
    does not order itself with a non-blocking stream, so the op reads the poisoned buffer: a mismatch, with the call pending.
    (Tried on up to eight fresh streams: one that shares the default stream's hardware queue cannot show it.)"""
    rs = sc.positive_control()
    for r in rs:
        print(sc.row("wrong_stream_op (control)", r))
        assert r.repeats and r.pending
    assert not rs[-1].bitwise, f"the planted wrong-stream op went unseen on {len(rs)} side streams"


def test_allowlist_names_only_known_cases():
    assert set(sc.HOST_SYNCHRONISING) <= set(sc.CASES)
    assert all(":" in reason for reason in sc.HOST_SYNCHRONISING.values())


@pytest.mark.parametrize("case", [c for c in sc.CASES if c not in sc.TRAINING])
def test_inference_entry_behind_pending_work(case):
    sc.check(case)


@pytest.mark.grad
@pytest.mark.parametrize("case", [c for c in sc.CASES if c in sc.TRAINING])
def test_training_entry_behind_pending_work(case):
    sc.check(case)
