"""Region-of-interest decode, the part that needs no GPU: the argument check of TensorDecoder.decode(roi=...) and the C surface."""
import os
import re

import pytest

import helpers

NEW = ("mij_batch_set_roi", "mij_batch_set_roi_auto", "mij_batch_slot_roi_rect")


@pytest.mark.parametrize("bad", (1, 0, None, "yes", [True], (0, 0, 8, 8)))
def test_decode_refuses_a_roi_that_is_no_bool(ica, bad):
    """before any device call: the decoder has no context, no batch and no device index afterwards, and the streams were not even parsed"""
    import torch  # noqa: F401  (the decoder module needs it)
    dec = ica.TensorDecoder("cuda")
    with pytest.raises(ValueError, match="roi"):
        dec.decode([b"not a jpeg"], crops=[(0, 0, 8, 8)], roi=bad)
    assert dec._ctx is None and dec._batch is None and dec._dev.index is None


def test_new_symbols_are_declared_and_exported(ica):
    src = open(os.path.join(helpers.ROOT, "include", "mij.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"^int\s+(mij_\w+)\s*\(", src, flags=re.M))
    L = ica.lib()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
