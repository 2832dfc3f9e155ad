"""The module-scoped `ctx` fixture of the GPU tests, stated once: an up-to-date build (build() of an up-to-date tree compares file times
and compiles nothing) and one Context on device 0, closed when the requesting module is done.  A test module takes it with
`from gpu_context import ctx  # noqa: F401`; pytest then makes one per requesting module."""
import pytest


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from vorbispizza_amd import Context
    c = Context(0)
    yield c
    c.close()
