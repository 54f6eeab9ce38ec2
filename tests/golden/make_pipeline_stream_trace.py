"""Writes tests/golden/pipeline_stream_trace.json: the ordered stream operations of ``TwoStreamPipeline`` in the scenarios
of ``tests/test_pipeline_order_host.py``, recorded with that test's own recorder (no GPU is needed).

    python tests/golden/make_pipeline_stream_trace.py

The file pins the choreography of the commit it was recorded from: re-record it only for a change that is meant to move an
operation, and read the diff line by line when you do.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import test_pipeline_order_host as order  # noqa: E402

if __name__ == "__main__":
    text = order.render({s.__name__: order.record(s) for s in order.SCENARIOS})
    with open(order.GOLDEN, "w") as f:
        f.write(text)
    print("%s: %d lines" % (order.GOLDEN, text.count("\n")))
