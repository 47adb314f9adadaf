"""CPU tests of the checkpoint path's host side (no device): the evaluator that keeps every `every`-th state
(vdf_minroot_eval_checkpoints) and the circuits made from such states (vdf_nova_circuits_from_checkpoints), against the
host's own full trace, against oracle/pasta.py, and against eval_and_make_circuits on the same initial state.  Every
comparison is of bytes (canonical Montgomery form)."""
import ctypes as C

import numpy as np
import pytest

from oracle import pasta as o
from vdf_amd.hip import VdfError
from vdf_amd.minroot import EvalMode, PallasVDF, State, VestaVDF, FIELD_FQ, _Fe, _State, nova_lib
from vdf_amd.nova import InverseMinRootCircuit

MODE_NAMES = {EvalMode.LTRSequential: "LTRSequential", EvalMode.LTRAddChainSequential: "LTRAddChainSequential",
              EvalMode.RTLSequential: "RTLSequential", EvalMode.RTLAddChainSequential: "RTLAddChainSequential"}
CASES = [(PallasVDF, m) for m in EvalMode.all()] + [(VestaVDF, EvalMode.LTRSequential)]


def initial(V, seed=11, i0=1):
    m = o.modulus(V.FIELD)
    return o.rand_fe(seed, 0, m), o.rand_fe(seed, 1, m), i0


def host_trace_states(vdf, s0, t):
    """the states vdf_minroot_eval's trace holds: (x, y) from the trace, i = i0 + k"""
    V = type(vdf)
    buf = np.zeros((t + 1, 2, 4), dtype="<u8")
    out = _State()
    assert nova_lib.vdf_minroot_eval(V.FIELD, int(vdf.eval_mode), C.byref(s0._c()), t, C.byref(out), buf.ctypes.data) == 0
    i0 = s0.to_ints(V.FIELD)[2]
    return [State(buf[k, 0].tobytes(), buf[k, 1].tobytes(), V.element(i0 + k)) for k in range(t + 1)]


@pytest.mark.parametrize("V,mode", CASES)
@pytest.mark.parametrize("every", [1, 8, 96])
def test_eval_checkpoints_equals_the_trace_and_the_oracle(V, mode, every):
    t_total = 96
    ints = initial(V)
    s0 = State.from_ints(V.FIELD, *ints)
    vdf = V.new_with_mode(mode)
    got = vdf.eval_checkpoints(s0, t_total, every)
    assert len(got) == t_total // every + 1
    full = host_trace_states(vdf, s0, t_total)
    assert got == full[::every]
    assert got[0] == s0 and got[-1] == vdf.eval(s0, t_total)
    want = o.minroot_eval_trace(o.State(*ints), t_total, V.FIELD, MODE_NAMES[mode])[::every]
    assert [s.to_ints(V.FIELD) for s in got] == [(w.x, w.y, w.i) for w in want]


@pytest.mark.parametrize("every", [0, 5, 97, 192])
def test_eval_checkpoints_refuses_an_interval_that_does_not_divide(every):
    s0 = State.from_ints(FIELD_FQ, *initial(PallasVDF))
    out = (_State * 200)()
    rc = nova_lib.vdf_minroot_eval_checkpoints(FIELD_FQ, 0, C.byref(s0._c()), 96, every, out)
    assert rc == 1                                                    # VDF_ERR_BAD_ARG
    with pytest.raises(ValueError):
        PallasVDF.new().eval_checkpoints(s0, 96, every)
    assert nova_lib.vdf_minroot_eval_checkpoints(FIELD_FQ, 0, None, 96, 8, out) == 1
    assert nova_lib.vdf_minroot_eval_checkpoints(FIELD_FQ, 0, C.byref(s0._c()), 96, 8, None) == 1
    assert nova_lib.vdf_minroot_eval_checkpoints(7, 0, C.byref(s0._c()), 96, 8, out) == 1


def oracle_states(ints, t_total, every):
    tr = o.minroot_eval_trace(o.State(*ints), t_total, o.FIELD_FQ)[::every]
    return [State.from_ints(FIELD_FQ, s.x, s.y, s.i) for s in tr]


@pytest.mark.parametrize("every", [24, 8])
def test_from_checkpoints_equals_eval_and_make_circuits(every):
    t, n = 24, 5
    ints = initial(PallasVDF, seed=5)
    s0 = State.from_ints(FIELD_FQ, *ints)
    states = oracle_states(ints, t * n, every)
    z0_a, ca = InverseMinRootCircuit.eval_and_make_circuits(PallasVDF.new(), t, n, s0)
    z0_b, cb = InverseMinRootCircuit.from_checkpoints(t, every, n, states)
    assert len(ca) == len(cb) == n
    assert z0_a == z0_b == [states[-1].x, states[-1].y, states[-1].i]
    for k in range(n):
        assert ca.states(k) == cb.states(k)
    # fresh checkpoint circuits hold no trace anywhere
    assert cb.memory() == (0, 0)
    assert cb.trace_ptr(0) is None
    ca.free(); cb.free()


@pytest.mark.parametrize("every", [24, 8])
@pytest.mark.parametrize("where", ["first+1", "middle", "last"])
def test_from_checkpoints_names_the_state_whose_counter_is_off(every, where):
    t, n = 24, 5
    ints = initial(PallasVDF, seed=5)
    states = oracle_states(ints, t * n, every)
    k = {"first+1": 1, "middle": len(states) // 2, "last": len(states) - 1}[where]
    x, y, i = states[k].to_ints(FIELD_FQ)
    states[k] = State.from_ints(FIELD_FQ, x, y, i + 1)
    with pytest.raises(VdfError) as e:
        InverseMinRootCircuit.from_checkpoints(t, every, n, states)
    assert e.value.code == 1
    msg = nova_lib.vdf_nova_last_error().decode()
    assert ("checkpoint %d:" % k) in msg


def test_from_checkpoints_bad_arguments():
    t, n = 24, 5
    states = oracle_states(initial(PallasVDF, seed=5), t * n, 24)
    raw = b"".join(s.x + s.y + s.i for s in states)
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    z0 = C.byref((_Fe * 3)())
    h = C.c_void_p()
    f = nova_lib.vdf_nova_circuits_from_checkpoints
    assert f(t, 24, 0, buf, z0, C.byref(h)) == 1                  # num_steps = 0
    assert f(t, 24, n, None, z0, C.byref(h)) == 1                 # null states
    assert f(t, 24, n, buf, None, C.byref(h)) == 1                                    # null z0
    assert f(t, 24, n, buf, z0, None) == 1                        # null out
    assert f(t, 0, n, buf, z0, C.byref(h)) == 1                   # every = 0
    assert f(t, 7, n, buf, z0, C.byref(h)) == 1                   # every does not divide t
    assert f(0, 24, n, buf, z0, C.byref(h)) == 1                  # t = 0
    assert h.value is None
    m = nova_lib.vdf_nova_circuits_memory
    assert m(None, None, None) == 1


def test_memory_of_fresh_checkpoint_circuits_is_zero():
    t, n = 24, 5
    states = oracle_states(initial(PallasVDF, seed=9), t * n, 8)
    _z0, c = InverseMinRootCircuit.from_checkpoints(t, 8, n, states)
    steps, nbytes = C.c_size_t(99), C.c_uint64(99)
    assert nova_lib.vdf_nova_circuits_memory(c.handle, C.byref(steps), C.byref(nbytes)) == 0
    assert (steps.value, nbytes.value) == (0, 0)
    # releasing what was never materialised is a no-op
    c.release()
    assert c.memory() == (0, 0)
    c.free()
