"""CPU only: every refusal, limit and early-out include/hv_kernels.h documents, checked on the host half of each entry point.

The argument checks, grid sizing and workspace rules of libhv_kernels.so are plain C++.  On a machine without a GPU a call that passes
every guard reaches its launch and returns -2, a refused call returns -1 before any launch, a documented early-out returns 0 - so the
table of tests/abi_contract.py can be run with made-up pointers.  Where a GPU exists this file is skipped BEFORE the library is
loaded: a missing guard would launch a kernel on those pointers, and that must never reach a real device (accepted calls are run on
the GPU by tests/test_gpu_abi_boundaries.py)."""
import os

import pytest

if os.path.exists("/dev/kfd"):
    pytest.skip("a GPU is present: calls with made-up pointers must not reach a device", allow_module_level=True)

from hunyuanvideo_efficiency_amd import _abi, _lib  # noqa: E402
from tests import abi_contract as T  # noqa: E402

ROWS = T.rows()


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name,overrides,want", [pytest.param(n, ov, w, id=i) for i, n, ov, w in ROWS])
def test_row(lib, name, overrides, want):
    """baseline: -2 (accepted, the launch fails without a device); refusal: -1; accept / last value inside a limit: -2; early-out: 0"""
    assert T.call(lib, name, overrides) == want


def test_every_stream_entry_point_has_a_baseline_and_nothing_else_is_listed():
    decls = T.stream_decls()
    assert set(T.E) == set(decls), (sorted(set(decls) - set(T.E)), sorted(set(T.E) - set(decls)))
    all_names = {name for _, name, _ in _abi.DECLS}
    for listed in (T.QUERIES, {k: 0 for k, *_ in T.SIZE_RULES}, {r[2]: 0 for r in T.SIZE_RULES}, {n: 0 for n, _ in T.NOT_DRIVEN}):
        assert set(listed) <= all_names, sorted(set(listed) - all_names)
    # the queries are exactly the declarations without a stream that take arguments
    assert set(T.QUERIES) == {name for _, name, params in _abi.DECLS if name not in decls and params}
    assert len(T.NOT_DRIVEN) <= 5


def test_every_parameter_of_every_baseline_is_a_parameter_and_every_pointer_is_classified():
    for name, params in T.stream_decls().items():
        e = T.E[name]
        assert list(e.base) and set(e.base) == {p for t, p in params if t != "hipStream_t"}, name
        ptrs = T.pointer_params(params)
        assert sorted(e.required + e.nullable) == sorted(ptrs), (name, ptrs)
        assert not set(e.required) & set(e.nullable), name
        assert all(e.base[p] is not None for p in e.required), name
        assert e.refuse or e.limits, name


def test_every_header_limit_is_used_by_a_limit_pair():
    used = {m for e in T.E.values() for _, macros, _, _ in e.limits for m in macros}
    assert used | set(T.MACROS_NOT_LIMITS) == set(_abi.MACROS), sorted(set(_abi.MACROS) ^ (used | set(T.MACROS_NOT_LIMITS)))
    assert not used & set(T.MACROS_NOT_LIMITS)


@pytest.mark.parametrize("name", sorted(T.QUERIES))
def test_host_query(lib, name):
    """0 for the shapes its kernel refuses, the documented value elsewhere, and never a negative number"""
    fn = getattr(lib, name)
    for args, want in T.QUERIES[name]:
        got = fn(*args)
        assert (got > 0) if want is None else (got == want), (name, args, got, want)
    for args in T.sweep(len(_lib.SIGNATURES[name])):
        assert fn(*args) >= 0, (name, args)


@pytest.mark.parametrize("query,qargs,kernel,param,scale", T.SIZE_RULES, ids=[r[0] for r in T.SIZE_RULES])
def test_size_query_is_the_kernels_own_minimum(lib, query, qargs, kernel, param, scale):
    size = getattr(lib, query)(*qargs) * scale
    assert size > 0
    assert T.call(lib, kernel, {param: size}) == T.LAUNCH
    assert T.call(lib, kernel, {param: size - 1}) == T.ARG
