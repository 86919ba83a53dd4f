"""RequestOptions.from_request (llava_mi355x/model.py) reads a scheduler request dict — as the request thread builds it and as it arrives over the
tensor-parallel command channel (tp_serving.CommandChannel.wire_request: host copies, tuples as lists) — into the same four fields.  No GPU."""
import torch


def _request(**extra):
    # the wire-format request of tests/test_tp_cpu.py::_channel_worker
    return dict({"ids": torch.arange(7)[None], "images": [torch.ones(3, 4, 4, dtype=torch.float16)], "attention_mask": None,
                 "sampling": (0.8, 0.9, None, 123456789012345), "prefill_chunk": 0}, **extra)


def test_from_request_reproduces_the_four_fields():
    from llava_mi355x.model import RequestOptions
    from llava_mi355x.tp_serving import CommandChannel
    assert RequestOptions() == (None, None, None, None) and RequestOptions._fields == ("sampling", "stop", "rules", "score_log")
    stop, rules = ([2, 7], [[5, 6, 7], [9]]), (1.3, 2, 4, [2], [11, 12])
    full = _request(stop=stop, rules=rules, score_log=(12, True), out_ref=[1, 2, 3])
    want = RequestOptions(sampling=(0.8, 0.9, None, 123456789012345), stop=stop, rules=rules, score_log=(12, True))
    for r in (full, CommandChannel.wire_request(full)):
        got = RequestOptions.from_request(r)
        assert got == want and all(isinstance(f, tuple) for f in got), got
        assert isinstance(got.sampling[3], int) and got.sampling[2] is None
    # absent keys, and keys that hold None, give None
    bare = _request()
    for r in (bare, CommandChannel.wire_request(bare)):
        assert RequestOptions.from_request(r) == RequestOptions(sampling=bare["sampling"])
    assert RequestOptions.from_request(dict(bare, sampling=None, stop=None)) == RequestOptions()
    assert RequestOptions.from_request({}) == RequestOptions()
