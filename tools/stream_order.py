"""Prints the table of profiles/stream_order.txt: every case of tests/stream_checks.py run behind pending work on a side stream
-- the calibrated delay, the host time the call took to return, whether the stream was still blocked when it returned
(pending), whether two default-stream runs agree (repeats), whether the side-stream outputs equal them bit for bit, and for the
entries that are documented to block the host the line that does.

    python tools/stream_order.py [case ...]
"""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import stream_checks as sc  # noqa: E402


def main(names):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    d = sc.delay()
    print(f"# {torch.cuda.get_device_name(0)}; delay kernel: {d.kind} x {d.count} = {d.ms:.1f} ms (target {sc.TARGET_MS:.0f} ms)")
    print(f"# GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES', 'unset')}: a wrong-stream launch that shares a hardware queue "
          "with the sleeping stream is not seen")
    rs = sc.positive_control()
    for r in rs:
        print(sc.row("wrong_stream_op (control)", r) + "  [must be: pending yes; bitwise no on one of up to 8 streams]")
    bad = int(not (all(r.pending for r in rs) and not rs[-1].bitwise))
    for name in names or list(sc.CASES):
        try:
            r = sc.behind_pending_work(sc.CASES[name]())
        except Exception:           # a Python error of one case: report it and go on (a GPU fault ends the process)
            print(f"{name:34s} ERROR\n{traceback.format_exc()}")
            bad += 1
            torch.cuda.synchronize()
            continue
        line = sc.row(name, r)
        ok = r.repeats and r.bitwise and (r.pending or name in sc.HOST_SYNCHRONISING)
        if not ok:
            bad += 1
            line += f"  <-- FAILS (outputs that differ: {r.mismatched} of {len(r.expected)})"
        print(line, flush=True)
    print(f"# {bad} failing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
