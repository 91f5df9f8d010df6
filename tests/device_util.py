"""Contexts for the -m gpu tests.  A test module imports the fixtures it uses by name; a module-scoped fixture imported that way is
set up once per importing module, so every module still opens and closes contexts of its own."""
import pytest

from multiclust_amd import hip


def status_of(rc):
    return hip.STATUS.get(rc, rc)


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def contexts():
    ctxs = [hip.Context(0) for _ in range(2)]
    yield ctxs
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def knob_contexts():
    """one Context per knob setting: nothing reuses buffers or a geometry that an older setting chose"""
    held = {}

    def get(knobs):
        key = tuple(sorted(knobs.items()))
        if key not in held:
            held[key] = hip.Context(0)
        return held[key]
    yield get
    for c in held.values():
        c.close()


def set_knobs(monkeypatch, knobs, all_knobs):
    """exactly these knobs in the environment, of all the library reads"""
    for k in all_knobs:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def snapshot(ctx, n_secants):
    """what an analysis must leave as it was: the data set, the counts, slots 0 to 2 and the first n_secants secants, as bytes"""
    out = [ctx.get_genotypes().tobytes(), ctx.expected_counts().tobytes(), repr(ctx.data_counts()), repr(ctx.empty_individuals())]
    for slot in range(3):
        out += [ctx.get_q(slot).tobytes(), ctx.get_p(slot).tobytes()]
    for j in range(n_secants):
        for which in (0, 1):
            p, q = ctx.get_secant(which, j)
            out += [p.tobytes(), q.tobytes()]
    return out
