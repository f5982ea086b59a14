"""Every torch custom op is held to the one argument contract of INTEGRATION.md ('Custom ops: what an op accepts') WITHOUT a GPU: the rows of
tests/ops_contract.py run through the undecorated implementations on meta tensors under the dry-run harness (the library replaced by a
recording stub), and through the registered fake rules on fake tensors.  A refusal must come by its exception type, name the op and the
operand, and reach no compute entry point; an accepted row must make exactly the op's entry points, each once, and return outputs of the
stated shapes and dtypes with contiguous strides.  The completeness check reads the registered schemas: an op added without rows fails here."""
import pytest
import torch

from tests import ops_contract as oc

ROWS = oc.rows()


@pytest.fixture(scope="module")
def ops():
    from probav_amd import ops
    return ops


@pytest.mark.parametrize("row", oc.refusal_rows(), ids=lambda r: r.id)
def test_refusal_names_the_operand_and_reaches_no_entry_point(ops, row):
    exc, calls, _ = oc.host_check(row)
    assert isinstance(exc, row.exc), "%s: expected %s, got %r" % (row.id, row.exc.__name__, exc)
    assert not isinstance(exc, NotImplementedError)
    assert calls == [], "%s reached %s before it was refused" % (row.id, calls)
    text = str(exc)
    assert row.case.op in text and row.operand in text, text
    if row.kind == "device":
        assert "no CPU fallback" in text, text
    if row.kind.startswith("dtype-"):
        assert row.kind.split("-", 1)[1] in text, text          # the dtype it got


@pytest.mark.parametrize("row", oc.accepted_rows(), ids=lambda r: r.id)
def test_accepted_row_makes_the_ops_entry_points_once_and_contiguous_outputs(ops, row):
    exc, calls, result = oc.host_check(row)
    assert exc is None, "%s was refused: %r" % (row.id, exc)
    assert sorted(calls) == sorted(row.entries) and len(set(calls)) == len(calls), (row.id, calls, row.entries)
    E = oc.Env("meta")
    want = row.outs if row.outs is not None else oc.expected_outs(row.case, row.case.args(E), E)
    oc.check_outputs(result, want, bool_mask=oc.bool_output(row))


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_wellformed_call_on_meta_tensors(ops, case):
    """The table's own well-formed call: accepted, its entry points each once, the stated outputs."""
    E = oc.Env("meta")
    with oc.dry_run() as stub:
        result = ops.IMPLS[case.op](*oc.values(case.args(E)))
    assert stub.calls == list(case.entries)
    oc.check_outputs(result, oc.expected_outs(case, case.args(E), E))


def _tensor_operands(case):
    return [n for n, v in case.args(oc.Env("meta")) if isinstance(v, torch.Tensor)]


@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.id)
def test_fake_rules_give_the_same_outcome(ops, case):
    """The same rows through the registered fake rules (FakeTensorMode, the dispatcher path): refused with the same exception type, or the
    outputs of the stated shapes, dtypes and strides.  A fake rule cannot know a HIP device from another: it sees that the operands agree, so
    the device row of an op with a single tensor operand is the one row it lets through (the real implementation refuses it)."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    alone = len(_tensor_operands(case)) == 1
    failures = []
    with oc.dry_run():
        ops.engine_sizes(oc.ENGINE["handle"])              # the engine is known to this process: the fake rules hold the operands to it
        for row in [r for r in ROWS if r.case is case]:
            with FakeTensorMode():
                E = oc.Env("fake")
                args = row.apply(E, case.args(E))
                refused = not row.accept and not (row.kind == "device" and alone)
                try:
                    result = getattr(torch.ops.probav, case.op)(*oc.values(args))
                except Exception as e:                     # noqa: BLE001
                    if not refused or not isinstance(e, row.exc):
                        failures.append("%s: %r" % (row.id, e))
                    continue
                if refused:
                    failures.append("%s: the fake rule let it through" % row.id)
                    continue
                try:
                    want = row.outs if row.outs is not None else oc.expected_outs(case, case.args(E), E)
                    oc.check_outputs(result, want, bool_mask=oc.bool_output(row))
                except AssertionError as e:
                    failures.append("%s: outputs %s" % (row.id, e))
    assert not failures, "\n".join(failures)


def _schema_ops():
    import probav_amd.ops  # noqa: F401
    return sorted(n.split("::")[1].split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith("probav::"))


def test_every_registered_op_has_its_plain_function_and_a_case(ops):
    names = set(_schema_ops())
    assert names and names == set(ops.IMPLS), names ^ set(ops.IMPLS)
    assert names == {c.op for c in oc.CASES}, names ^ {c.op for c in oc.CASES}


@pytest.mark.parametrize("name", _schema_ops())
def test_table_is_complete_for_every_tensor_argument_of_the_schema(ops, name):
    """For every Tensor / Tensor? argument of the registered schema: a device row, a dtype row, a layout row (accepted, or refused for an
    operand the op writes) and a size row.  Every operand the schema declares written is one the table refuses non-contiguous."""
    schema = getattr(torch.ops.probav, name).default._schema
    cases = [c for c in oc.CASES if c.op == name]
    kinds = {}
    for r in ROWS:
        if r.case.op == name:
            kinds.setdefault(r.operand, set()).add((r.kind.split("-")[0], r.accept))
    for a in schema.arguments:
        if str(a.type) not in ("Tensor", "Optional[Tensor]"):
            continue
        have = kinds.get(a.name, set())
        assert ("device", False) in have, (name, a.name, "no device row")
        assert ("dtype", False) in have, (name, a.name, "no dtype row")
        assert any(k == "size" for k, _ in have), (name, a.name, "no size row")
        written = a.alias_info is not None and a.alias_info.is_write
        if written or any(a.name in c.mutated for c in cases):
            assert all(a.name in c.mutated for c in cases if dict(c.args(oc.Env("meta"))).get(a.name) is not None), (name, a.name, "written by the schema, read in the table")
            assert ("noncontiguous", False) in have and ("offset", False) in have, (name, a.name, "no layout refusal")
        else:
            assert {("strided", True), ("offset", True)} <= have, (name, a.name, "no accepted layout rows")


def test_engine_sizes_are_asked_once_per_handle(ops):
    """The hot path gains no ctypes round trip per step: the second call of an engine op asks the library for nothing but its workspace."""
    E = oc.Env("meta")
    asked = []
    with oc.dry_run() as stub:
        for q in ("probav_param_count", "probav_weff_count", "probav_cout_total", "probav_weight_cache_bytes", "probav_layer_info", "probav_workspace_view"):
            inner = oc.QUERIES[q]
            stub.__dict__[q] = (lambda inner, q: lambda *a: (asked.append(q), inner(*a))[1])(inner, q)
        fwd, opt = oc.CASE["wdsr_forward+wcache"], oc.CASE["optimizer_wn_step"]
        ops.IMPLS["wdsr_forward"](*oc.values(fwd.args(E)))
        ops.IMPLS["optimizer_wn_step"](*oc.values(opt.args(E)))
        first = list(asked)
        ops.IMPLS["wdsr_forward"](*oc.values(fwd.args(E)))
        ops.IMPLS["optimizer_wn_step"](*oc.values(opt.args(E)))
        assert first and asked == first, (first, asked[len(first):])
        ops.forget_engine(oc.ENGINE["handle"])             # a re-routed or destroyed engine is asked again
        ops.IMPLS["wdsr_forward"](*oc.values(fwd.args(E)))
        assert len(asked) > len(first)


def test_dry_run_restores_what_it_replaced(ops):
    from probav_amd import _lib
    before = (_lib.lib, _lib.ptr, _lib.current_stream, _lib.require_device, ops._ws_pool, torch.cuda.use_mem_pool, dict(ops._ENGINE_SIZES))
    with oc.dry_run():
        ops.engine_sizes(oc.ENGINE["handle"])
    assert before == (_lib.lib, _lib.ptr, _lib.current_stream, _lib.require_device, ops._ws_pool, torch.cuda.use_mem_pool, dict(ops._ENGINE_SIZES))
