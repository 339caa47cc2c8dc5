"""What the argument-check tests (tests/test_small_kernels.py, tests/test_ops_arguments.py) share: sentinel-filled parent buffers and the
`rejects` assertion.  The rejection cases hand a wrapper views into larger allocations (never an undersized allocation, never pageable host
memory), so that even a missing check could not make a kernel touch memory the test does not own; behind every rejection the parent still
holds its fill, which shows that nothing was launched."""
import pytest
import torch

FILL = 123.0            # what the rejection cases fill their parents with
FILL16 = 0x5A5A         # the same for bf16 buffers, as a bit pattern


def sentinel16(shape, dev):
    return torch.full(tuple(shape), FILL16, dtype=torch.int16, device=dev).view(torch.bfloat16)


def holds16(t):
    return bool((t.view(torch.int16) == FILL16).all())


def rejects(ops_call, *parents):
    """ops_call raises MoviigenHipError and no parent buffer changed"""
    from wan.backend import lib
    with pytest.raises(lib.MoviigenHipError):
        ops_call()
    torch.cuda.synchronize()
    for p in parents:
        assert holds16(p) if p.dtype == torch.bfloat16 else bool((p == FILL).all()), 'a rejected call wrote to its output'


def host(t):
    """the tensor in pinned host memory: not a CUDA tensor for the wrapper, yet memory the device may touch"""
    return t.cpu().pin_memory()
