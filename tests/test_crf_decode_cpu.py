"""CPU: the host side of device-resident CRF decoding -- splitting ``tags_flat`` by ``lens`` (crf.DeviceTags.tolist), the
argument checks of icka_crf_score_decode's outputs, and what GraphedModule(decode=) accepts as a captured call's output."""
import pytest
import torch

from icka_amd import crf, kernels


def _dt(lens, flat, joint=False):
    if joint:
        buf = torch.tensor(list(lens) + list(flat), dtype=torch.int32)
        return crf.DeviceTags(buf[:len(lens)], buf[len(lens):], _joint=buf)
    return crf.DeviceTags(torch.tensor(lens, dtype=torch.int32), torch.tensor(flat, dtype=torch.int32))


@pytest.mark.parametrize("joint", [False, True])
def test_split_by_lens(joint):
    # ragged, with a trailing unused tail of the capacity (B*S = 3*4 = 12 entries, 7 used)
    t = _dt([3, 1, 3], [0, 1, 2, 5, 4, 4, 3, 9, 9, 9, 9, 9], joint)
    assert t.tolist() == [[0, 1, 2], [5], [4, 4, 3]]
    # empty masks give empty paths (the split itself; the kernel writes at least one tag per sample)
    assert _dt([0, 2, 0], [7, 8, 0, 0, 0, 0], joint).tolist() == [[], [7, 8], []]
    # full masks: the whole capacity is used
    assert _dt([2, 2], [1, 2, 3, 4], joint).tolist() == [[1, 2], [3, 4]]
    # B = 1
    assert _dt([1], [6], joint).tolist() == [[6]]
    assert _dt([4], [6, 5, 4, 3], joint).tolist() == [[6, 5, 4, 3]]


def test_split_tags_rejects_lengths_that_do_not_fit():
    with pytest.raises(ValueError):
        crf.split_tags([3, 2], [0, 1, 2, 3])
    with pytest.raises(ValueError):
        crf.split_tags([-1], [0])
    assert crf.split_tags([], []) == []


def test_device_tags_empty_is_one_buffer():
    t = crf.DeviceTags.empty(3, 5, "cpu")
    assert t.batch_size == 3 and t.capacity == 15
    assert t.lens.dtype == torch.int32 and t.tags_flat.dtype == torch.int32
    assert t._joint.numel() == 18 and t.tags_flat.data_ptr() == t.lens.data_ptr() + 3 * 4
    t.lens.copy_(torch.tensor([1, 5, 2], dtype=torch.int32))
    t.tags_flat[:8].copy_(torch.arange(8, dtype=torch.int32))
    assert t.tolist() == [[0], [1, 2, 3, 4, 5], [6, 7]]


def test_device_tags_argument_errors():
    i32 = torch.int32
    with pytest.raises(ValueError):                    # wrong dtype
        crf.DeviceTags(torch.zeros(2, dtype=torch.int64), torch.zeros(8, dtype=i32))
    with pytest.raises(ValueError):
        crf.DeviceTags(torch.zeros(2, dtype=i32), torch.zeros(8, dtype=torch.float32))
    with pytest.raises(ValueError):                    # wrong shape
        crf.DeviceTags(torch.zeros(2, 1, dtype=i32), torch.zeros(8, dtype=i32))
    with pytest.raises(ValueError):
        crf.DeviceTags(torch.zeros(2, dtype=i32), torch.zeros(2, 4, dtype=i32))
    with pytest.raises(ValueError):                    # not contiguous
        crf.DeviceTags(torch.zeros(4, dtype=i32)[::2], torch.zeros(8, dtype=i32))
    with pytest.raises(TypeError):
        crf.DeviceTags([0, 0], torch.zeros(8, dtype=i32))
    t = crf.DeviceTags(torch.zeros(2, dtype=i32), torch.zeros(8, dtype=i32))
    t.check(2, 4)                                      # capacity exactly B*S
    with pytest.raises(ValueError, match="needs up to 10"):
        t.check(2, 5)                                  # capacity too small
    with pytest.raises(ValueError, match="lens holds 2 entries"):
        t.check(3, 2)                                  # batch size does not match lens
    with pytest.raises(ValueError):
        kernels.check_flat_tags(torch.zeros(2, dtype=i32), torch.zeros(7, dtype=i32), 2, 4)


def test_device_decode_switch_nests_and_restores():
    assert not crf.device_decode_active()
    with crf.device_decode():
        assert crf.device_decode_active()
        with crf.device_decode():
            assert crf.device_decode_active()
        assert crf.device_decode_active()
    assert not crf.device_decode_active()
    with pytest.raises(RuntimeError):
        with crf.device_decode():
            raise RuntimeError("inside")
    assert not crf.device_decode_active()


def test_graphed_module_output_rules():
    from icka_amd.graph import _split_output
    t = _dt([1], [0])
    loss = torch.zeros(())
    logits = torch.zeros(2, 3)
    assert _split_output(logits, False) == (None, logits)
    assert _split_output(logits, True) == (None, logits)
    assert _split_output(t, True) == (t, None)
    assert _split_output((t, loss), True) == (t, loss)
    for out in (t, (t, loss), [[0]], ([[0]], loss)):
        with pytest.raises(TypeError):                 # decode=False: only one floating-point tensor (unchanged)
            _split_output(out, False)
    for out in ([[0]], ([[0]], loss), (t, torch.zeros(1, dtype=torch.int64)), (t, loss, loss)):
        with pytest.raises(TypeError):
            _split_output(out, True)
    with pytest.raises(TypeError):                     # a dev loss that feeds autograd is not captured
        _split_output((t, torch.zeros((), requires_grad=True)), True)
