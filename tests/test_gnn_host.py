"""CPU-only: the host side of the GNN layers (csrc/gnn.hip) - what its workspace queries answer, value for value, and what its entries
refuse, word for word (pats_last_error) and in which order.  The method of test_host_refusals_backend.py: the entries are called
through ctypes with made-up aligned addresses, which are not memory, so EVERY call here is one the host checks answer before anything
touches a device.  The one piece of real memory is the host struct pats_propagation_weights, whose fields the entry reads."""
import ctypes

import pytest

OK, INVALID, UNSUPPORTED = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from pats_amd import build, _lib
    build.build()
    return _lib.lib()


def address(k):
    """A made-up address for argument k: 256-byte aligned, none of them memory."""
    return 0x7f0000000000 + 0x100 * (k + 1)


def weights(null_field=None):
    """pats_propagation_weights on the host: fourteen pointers (include/pats_amd.h), all made-up addresses but `null_field`."""
    w = (ctypes.c_void_p * 14)(*[address(100 + k) for k in range(14)])
    if null_field is not None:
        w[null_field] = None
    return w


# ---- the sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args, size", [((0, 128, 65, 65), 2099456), ((1, 128, 65, 65), 2332416), ((3, 264, 145, 145), 9015808),
                                        ((5, 64, 20, 33), 1262336), ((-1, 128, 65, 65), 0), ((2, 128, 0, 5), 0)])
def test_layer_workspace_bytes(lib, args, size):
    assert lib.pats_attentional_propagation_workspace_bytes(*args) == size


@pytest.mark.parametrize("args, size", [((1, 264, 4, 145), 7486464), ((3, 264, 4, 145), 13792000), ((0, 264, 4, 145), 0),
                                        ((3, 128, 4, 65), 0), ((3, 264, 2, 145), 0)])
def test_stack_workspace_bytes(lib, args, size):
    assert lib.pats_attentional_gnn_packed_workspace_bytes(*args) == size


def test_building_block_workspace_bytes(lib):
    assert lib.pats_bn_fold_workspace_bytes(0) == 0
    assert lib.pats_bn_fold_workspace_bytes(256) == 262144
    assert lib.pats_conv1x1_workspace_bytes() == 256


# ---- the three layer entries ------------------------------------------------------------------------------------------------------
# entry -> (the name its own messages carry, its arguments in the order of the C signature)
LAYER = {
    "pats_attentional_propagation_f32": (
        None, "x source batch C heads n m w bn_train bn_eps residual out workspace workspace_bytes stream"),
    "pats_attentional_propagation_packed_f32": (
        "attentional_propagation_packed", "x source batch C heads n m w packed bn_train bn_eps residual out workspace workspace_bytes stream"),
    "pats_attentional_propagation_packed_counted_f32": (
        "attentional_propagation_packed_counted",
        "x source batch live live_off C heads n m w packed bn_train bn_eps residual out workspace workspace_bytes stream"),
}
LAYER_SCALARS = {"batch": 3, "C": 128, "heads": 4, "n": 65, "m": 65, "bn_train": 0, "bn_eps": 1e-5, "live_off": 0, "stream": None,
                 "live": None, "residual": None}
COUNTED_BN = ("attentional_propagation_packed_counted: bn_train with a device-side count is not supported (the batch statistics would take "
              "in the rows past the count)")
# what the shared checks turn away, in the order they are made (csrc/gnn.hip, propagation_impl): (what is wrong, the message, or None
# where the call returns 0 at once)
LAYER_CHECKS = [
    ({"C": 130}, "attentional_propagation: bad shape"),
    ({"C": 132}, "attentional_propagation: feature_dim must be a multiple of 8 (operand slabs of 8 channels)"),
    ({"batch": 0}, None),
    ({"x": None}, "attentional_propagation: null pointer"),
    ({"w": "one field null"}, "attentional_propagation: null weight pointer"),
    ({"workspace_bytes": 16}, "attentional_propagation: workspace too small"),
]


def layer_call(lib, entry, **kw):
    names = LAYER[entry][1].split()
    a = {n: LAYER_SCALARS[n] if n in LAYER_SCALARS else address(k) for k, n in enumerate(names)}
    a["workspace_bytes"] = lib.pats_attentional_propagation_workspace_bytes(3, 128, 65, 65)
    held = a["w"] = weights()
    for n, v in kw.items():
        assert n in a, n
        a[n] = v
    if a["w"] == "one field null":
        held = a["w"] = weights(null_field=7)
    args = [ctypes.cast(a[n], ctypes.c_void_p) if isinstance(a[n], ctypes.Array) else a[n] for n in names]
    rc = getattr(lib, entry)(*args)
    del held
    return rc


def answered(lib, entry, message, **kw):
    """The host checks answer the call: refused (PATS_ERR_INVALID) with exactly this message, or - message None - 0 at once."""
    rc = layer_call(lib, entry, **kw)
    if message is None:
        assert rc == OK, "%s(%s): %d" % (entry, kw, rc)
    else:
        assert rc == INVALID, "%s(%s) was not refused: %d" % (entry, kw, rc)
        assert lib.pats_last_error().decode() == message, kw


@pytest.mark.parametrize("entry", sorted(LAYER))
def test_layer_refusals(lib, entry):
    for wrong, message in LAYER_CHECKS:
        answered(lib, entry, message, **wrong)


@pytest.mark.parametrize("entry", sorted(LAYER))
def test_layer_the_earlier_check_wins(lib, entry):
    for i, (first, message) in enumerate(LAYER_CHECKS):
        for later, _ in LAYER_CHECKS[i + 1:]:
            if set(first) & set(later):
                continue                                # C = 130 and C = 132 are one argument
            answered(lib, entry, message, **dict(later, **first))


def test_the_packed_entries_checks_come_first(lib):
    """null packed weights, then (counted) batch statistics with a count, then the shared checks - whatever else is wrong"""
    for entry in ("pats_attentional_propagation_packed_f32", "pats_attentional_propagation_packed_counted_f32"):
        message = "%s: null packed weights" % LAYER[entry][0]
        answered(lib, entry, message, packed=None)
        for wrong, _ in LAYER_CHECKS:
            answered(lib, entry, message, packed=None, **wrong)
    counted = "pats_attentional_propagation_packed_counted_f32"
    answered(lib, counted, COUNTED_BN, live=address(60), bn_train=1)
    answered(lib, counted, "attentional_propagation_packed_counted: null packed weights", packed=None, live=address(60), bn_train=1)
    for wrong, _ in LAYER_CHECKS:
        answered(lib, counted, COUNTED_BN, live=address(60), bn_train=1, **wrong)
    # without a count batch statistics are taken: the shared checks answer
    answered(lib, counted, "attentional_propagation: workspace too small", bn_train=1, workspace_bytes=16)


# ---- the stack ------------------------------------------------------------------------------------------------------------------------
STACK = "desc0 desc1 batch live live_off C heads n layers weights packed cross bn_eps out0 out1 workspace workspace_bytes stream".split()
STACK_SCALARS = {"batch": 3, "live": None, "live_off": 0, "C": 264, "heads": 4, "n": 145, "layers": 1, "bn_eps": 1e-5, "stream": None}
# in the order the entry checks (csrc/gnn.hip, pats_attentional_gnn_packed_f32): (what is wrong, return code, message)
STACK_CHECKS = [
    ({"batch": -1}, INVALID, "attentional_gnn_packed: bad shape"),
    ({"C": 128, "n": 65}, UNSUPPORTED, None),
    ({"batch": 0}, OK, None),
    ({"weights": None, "packed": None, "cross": None}, INVALID, "attentional_gnn_packed: null pointer"),
    ({"out1": "desc0"}, INVALID, "attentional_gnn_packed: the outputs must not alias the inputs"),
    ({"workspace_bytes": 16}, INVALID, "attentional_gnn_packed: workspace too small"),
]


def stack_answered(lib, rc_want, message, **kw):
    a = {n: STACK_SCALARS[n] if n in STACK_SCALARS else address(k) for k, n in enumerate(STACK)}
    a["workspace_bytes"] = lib.pats_attentional_gnn_packed_workspace_bytes(3, 264, 4, 145)
    a.update(kw)
    if a["out1"] == "desc0":
        a["out1"] = a["desc0"]
    rc = lib.pats_attentional_gnn_packed_f32(*[a[n] for n in STACK])
    assert rc == rc_want, "gnn_packed(%s): %d" % (kw, rc)
    if message is not None:
        assert lib.pats_last_error().decode() == message, kw


@pytest.mark.parametrize("C, heads, n", [(128, 4, 65), (264, 2, 145), (264, 4, 144), (64, 4, 20), (256, 4, 145)])
def test_stack_is_unsupported_at_any_other_shape(lib, C, heads, n):
    stack_answered(lib, UNSUPPORTED, None, C=C, heads=heads, n=n)


def test_stack_refusals(lib):
    for wrong, rc, message in STACK_CHECKS:
        stack_answered(lib, rc, message, **wrong)


def test_stack_the_earlier_check_wins(lib):
    for i, (first, rc, message) in enumerate(STACK_CHECKS):
        for later, _, _ in STACK_CHECKS[i + 1:]:
            if set(first) & set(later):
                continue                                # batch = -1 and batch = 0 are one argument
            stack_answered(lib, rc, message, **dict(later, **first))
