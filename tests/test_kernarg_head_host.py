"""Kernel-argument preload, read back from the built library (no GPU): the
kernels whose leading plain parameters arrive in SGPRs (k_row2's four
instances: csrc/sa_row2.hip, the one unit csrc/Makefile builds with the
preload flag) have a preload length > 0 in their kernel descriptors, every
other kernel of libsparc_amp.so has 0.  Skips where no library is built."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "sparc_ldpc_amd", "libsparc_amp.so")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

# demangled-name prefixes of the kernels with a head of plain parameters
HEAD_KERNELS = ("void sa::k_row2<",)
HEAD_INSTANCES = 4  # <float | double, 16 | 32 rows, 512 threads>


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libsparc_amp.so is not built")
    import kres
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump"):
        if not os.path.exists(os.path.join(kres.LLVM, tool)):
            pytest.skip(f"{tool} not found")
    ks = kres.library_kernels(LIB)
    names = kres.demangle(ks)
    return {names.get(k, k): v for k, v in ks.items()}


def test_library_lists_its_kernels(kernels):
    assert len(kernels) > 100, len(kernels)  # the section, row, dense, glue, Monte-Carlo and state-evolution kernels
    assert all(size > 0 for size, _ in kernels.values())


def test_head_kernels_are_preloaded(kernels):
    head = {k: v for k, v in kernels.items() if k.startswith(HEAD_KERNELS)}
    assert len(head) == HEAD_INSTANCES, sorted(head)
    for name, (size, pre) in head.items():
        assert pre == 14, (name, pre)     # the whole head: 14 dwords is the hardware's limit
        assert size <= 128, (name, size)  # head + tail in two 64-byte lines


def test_every_other_kernel_is_not(kernels):
    rest = {k: v for k, v in kernels.items() if not k.startswith(HEAD_KERNELS)}
    assert rest
    assert [k for k, (_, pre) in rest.items() if pre != 0] == []
