"""Device arrays between guard words, for the tests that call kernels straight through the C ABI (tests/test_hip_seq_f64.py,
tests/test_hip_ppo_f64.py): every array is a view into a larger allocation with GUARD words of a NaN bit pattern on each side, so a
store outside the array shows as a changed guard word and an element a kernel leaves unwritten shows as a NaN."""
import torch

DEV = "cuda:0"
GUARD = 64               # floats on each side of every array
NAN_BITS = 0x7FC0BEEF    # a quiet NaN with a payload no arithmetic produces


def guarded(shape, data=None):
    """-> (the whole allocation as int32, the float32 view of `shape` in its middle)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + n].view(torch.float32).view(*shape)
    assert view.data_ptr() % 16 == 0
    if data is not None:
        view.copy_(data)
    return buf, view


def guarded_like(data):
    """`guarded` for an array of any element type (int64 row indices, uint8 flags): -> (the allocation as int32, a view of data's type
    and shape holding `data`).  The array is rounded up to whole words; `words_of` gives that count."""
    nbytes = data.numel() * data.element_size()
    buf = torch.full((words_of(data) + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + words_of(data)].view(torch.uint8)[:nbytes].view(data.dtype).view(*data.shape)
    view.copy_(data)
    return buf, view


def words_of(view):
    return (view.numel() * view.element_size() + 3) // 4


def guard_problem(name, buf, view):
    """None, or what happened to the guard words around `view`"""
    lo, hi = buf[:GUARD], buf[GUARD + words_of(view):]
    assert hi.numel() == GUARD, (name, hi.numel())
    if bool((lo == NAN_BITS).all()) and bool((hi == NAN_BITS).all()):
        return None
    return f"guard of {name} touched ({int((lo != NAN_BITS).sum())} words below, {int((hi != NAN_BITS).sum())} above)"
