"""`hip_runtime.fanout.accumulate_in_place`: the slot form of a consumer that adds its share to what its output buffer
already holds (both DCN backwards, `_MaxPool.backward`, a head on the leading images).  Host logic only: CPU tensors, no
kernel is launched."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'centernet-uda_amd'))


def test_accumulate_in_place_hands_out_an_owned_buffer_only():
    from hip_runtime.fanout import GradSlot, accumulate_in_place
    assert accumulate_in_place(None) is None                      # the input was not forked

    slot = GradSlot()
    assert accumulate_in_place(slot) is None and slot.included == []      # nobody wrote yet: the consumer claims

    foreign = torch.zeros(2, 3)
    slot.buf, slot.owned = foreign, False                         # another consumer's own gradient tensor: not ours to add into
    assert accumulate_in_place(slot) is None
    assert not slot.has(foreign) and slot.buf is foreign and not slot.owned

    buf = torch.zeros(2, 3)
    slot.buf, slot.owned = buf, True
    assert accumulate_in_place(slot) is buf
    assert slot.has(buf) and slot.buf is buf and slot.owned       # recorded: _Fork.backward does not add it again


def test_accumulate_in_place_resolves_a_slot_merged_upwards():
    from hip_runtime.fanout import GradSlot, accumulate_in_place
    parent = GradSlot()
    inner = GradSlot(parent)
    inner._buf, inner._owned = torch.ones(2, 3), True             # (what the merge leaves behind is not looked at)
    inner.up = parent
    assert accumulate_in_place(inner) is None                     # the parent's total is empty
    buf = torch.zeros(2, 3)
    parent.buf, parent.owned = buf, True
    assert accumulate_in_place(inner) is buf
    assert parent.has(buf) and inner.has(buf) and parent._included[-1] is buf and inner._included == []
