"""The case table of the autograd-Function tests (tests/function_cases.py), checked on the CPU: every Function of the package
has a case (the inventory walks EVERY module of `cflearn_amd`, no module list), every float64 reference agrees with the torch call it
restates and passes gradcheck, every case names an error model for each of its outputs and differentiable inputs."""
import importlib
import importlib.machinery
import inspect
import pkgutil

import pytest
import torch

import function_cases as FC
from function_cases import CASES

NAMES = sorted(CASES)


def package_functions():
    """every `Function` subclass of the package, found in the module that defines it: the walk is over the package's own path,
    so a Function in a module added later is seen without anybody listing that module"""
    import cflearn_amd

    found = set()
    for info in pkgutil.iter_modules(cflearn_amd.__path__, cflearn_amd.__name__ + "."):
        spec = info.module_finder.find_spec(info.name)
        if not isinstance(spec.loader, importlib.machinery.SourceFileLoader):
            continue  # the built shared libraries beside the sources (the C library, the binding) hold no Python class
        mod = importlib.import_module(info.name)
        for obj in vars(mod).values():
            if inspect.isclass(obj) and issubclass(obj, torch.autograd.Function) and obj.__module__ == mod.__name__:
                found.add(obj)
    return found


def missing_functions(cases):
    covered = set(FC.WRAPPER_FNS)
    for c in cases:
        covered.update(c.fns)
    return sorted(f"{f.__module__.rsplit('.', 1)[-1]}.{f.__name__}" for f in package_functions() - covered)


def test_every_function_has_a_case():
    assert len(package_functions()) >= 62, "the introspection lost Function subclasses"
    missing = missing_functions(CASES.values())
    assert not missing, f"no case in tests/function_cases.py for: {', '.join(missing)}"


def test_the_inventory_notices_a_function_without_cases():
    """no exclusion list: a Function whose entries are gone is reported by name"""
    for fn in package_functions() - set(FC.WRAPPER_FNS):
        rest = [c for c in CASES.values() if fn not in c.fns]
        assert len(rest) < len(CASES), fn.__name__
        if not any(fn in c.fns for c in rest):
            assert any(m.endswith("." + fn.__name__) for m in missing_functions(rest)), fn.__name__


@pytest.mark.parametrize("name", NAMES)
def test_reference_restates_the_torch_call(name):
    c = CASES[name]
    assert c.obvious is not None, "every reference names the torch call it restates"
    v = FC.values64(c, c.make(), grad=False)
    got, want = FC.as_tuple(c.ref(v)), FC.as_tuple(c.obvious(v))
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and g.shape == w.shape, (g.dtype, g.shape, w.shape)
        # two float64 evaluations of one formula: a few hundred roundings of 2^-53 on values of order 1..100
        torch.testing.assert_close(g, w, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("name", NAMES)
def test_reference_passes_gradcheck(name):
    c = CASES[name]
    if not c.diff:
        return  # a forward-only case: nothing to differentiate
    vals = c.make()
    v = FC.values64(c, vals)
    wrt = [k for k in c.diff]

    def f(*xs):
        vv = dict(v)
        vv.update(dict(zip(wrt, xs)))
        return FC.as_tuple(c.ref(vv))

    # (the full Jacobian up to 1000 input elements, gradcheck's random projections of it beyond: the check stays under a second)
    fast = c.fast_gradcheck or sum(v[k].numel() for k in wrt) > 1000
    assert torch.autograd.gradcheck(f, tuple(v[k] for k in wrt), eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=fast, nondet_tol=0.0)


@pytest.mark.parametrize("name", NAMES)
def test_every_output_and_gradient_has_an_error_model(name):
    c = CASES[name]
    vals = c.make()
    ys0 = FC.as_tuple(c.ref(FC.values64(c, vals, grad=False)))
    dys = FC.make_dys(c, ys0, 1)
    ys, gs = FC.grads64(c, vals, dys)
    want = {f"y{i}" for i in range(len(ys))} | set(c.diff)
    assert set(c.err) == want, f"error models {sorted(c.err)} for outputs / inputs {sorted(want)}"
    assert len(c.out) == len(ys)
    assert set(c.params) <= set(c.diff) or c.name == "patch_tokens"
    if any(e.units == "mix" for e in c.err.values()):
        return
    for key, (ulps, units, dtype) in FC.bounds(c, vals, dys, ys, gs).items():
        ref = ys[int(key[1:])] if key[0] == "y" and key[1:].isdigit() else gs[key]
        assert bool((torch.as_tensor(ulps) >= 0).all()) and dtype in (torch.bfloat16, torch.float32)
        if isinstance(ulps, torch.Tensor):
            assert ulps.shape == ref.shape, (key, ulps.shape, ref.shape)
        if units is not None:
            assert torch.broadcast_shapes(units.shape, ref.shape) == ref.shape, (key, units.shape, ref.shape)
            assert bool(torch.isfinite(units).all()) and bool((units >= 0).all()), key


@pytest.mark.parametrize("name", sorted(FC.NBM_CASES))
def test_no_hidden_unit_of_a_bases_case_sits_on_its_kink(name):
    """the dyadic operands of the bases cases could give a pre-activation of exactly zero, where the reference's mask and a
    difference quotient disagree; the seeds are chosen so that none does (a non-zero pre1 is at least 2^-15 = 3e-5 away)"""
    assert FC.nbm_relu_margin(name) > 2e-5


def test_at_most_one_refused_combination_per_function():
    seen = {}
    for c in CASES.values():
        if c.refused is not None:
            for fn in c.fns:
                assert fn not in seen, f"{fn.__name__}: refused in {seen[fn]} and {c.name}"
                seen[fn] = c.name
