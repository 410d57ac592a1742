"""The public surface of the Ant System stack stays what it was when the bindings were three copies: the signatures of the
five bindings, ``heatmap_rollout`` and ``AntSystem`` against literals, and the family tables against the library's prototype
table and struct mirrors. No GPU, no library load."""
import ctypes
import inspect

import pytest

from rl4co_amd import _lib
from rl4co_amd import kernels as K
from rl4co_amd.aco import AntSystem, heatmap_rollout

_COMMON = ("alpha=1.0, beta=1.0, decay=0.95, Q=1.0, temperature=1.0, ln_noise=None, philox_seed=0, philox_offset=0, "
           "philox_seed_dev=None, forced_actions=None, actions=None, reward=None, final_reward=None, final_actions=None, ")
_RAGGED = "final_iteration=None, has_best=False, iteration_base=0, all_logps=False, record_iterations=False, "
SIGNATURES = {
    K.aco_tsp: "(pheromone, *, n_ants, phases=3, iterations=1, log_heuristic=None, locs=None, start_nodes=None, " + _COMMON
               + "has_best=False, all_logps=False, record_iterations=False, err=None)",
    K.aco_cvrp: "(pheromone, *, n_ants, phases=3, iterations=1, log_heuristic=None, locs=None, demand=None, "
                "vehicle_capacity=None, start_nodes=None, " + _COMMON + _RAGGED + "err=None)",
    K.aco_prize: "(pheromone, *, env, n_ants, phases=3, iterations=1, log_heuristic=None, locs=None, prize=None, penalty=None, "
                 "max_length=None, " + _COMMON + _RAGGED + "n_workgroups=0, err=None)",
    K.aco_tsp_logp_grad: "(heatmap, actions, grad_ll, *, grad_steps=None, temperature=1.0, row_split=None, "
                         "pos_in_scratch=None, err=None)",
    K.aco_depot_logp_grad: "(heatmap, actions, grad_ll, *, env, grad_steps=None, locs=None, demand=None, "
                           "vehicle_capacity=None, prize=None, max_length=None, multistart=False, temperature=1.0, "
                           "row_split=None, table_in_scratch=None, err=None)",
    heatmap_rollout: "(heatmap, locs, *, n_ants, start_nodes=None, actions=None, temperature=1.0, seed=None, err=None, "
                     "env_name='tsp', td=None)",
    AntSystem.__init__: "(self, log_heuristic, n_ants=20, alpha=1.0, beta=1.0, decay=0.95, Q=None, pheromone=None, "
                        "use_local_search=False, use_nls=False, n_perturbations=1, local_search_params={}, "
                        "perturbation_params={})",
    AntSystem.run: "(self, td_initial, env, n_iterations, decoding_kwargs, disable_tqdm=True)",
}


def _plain(fn) -> str:
    """The signature without annotations: names, order, kinds (the ``*``) and defaults."""
    sig = inspect.signature(fn)
    params = [p.replace(annotation=inspect.Parameter.empty) for p in sig.parameters.values()]
    return str(sig.replace(parameters=params, return_annotation=inspect.Signature.empty))


@pytest.mark.parametrize("fn", list(SIGNATURES), ids=lambda fn: fn.__qualname__)
def test_signature_is_the_parents(fn):
    assert _plain(fn) == SIGNATURES[fn]
    assert fn.__doc__ or fn is AntSystem.__init__ or fn is AntSystem.run


def _pointers_and_scalars(struct) -> tuple[set, set]:
    fields = dict(struct._fields_)
    pointers = {name for name, ctype in fields.items() if ctype is ctypes.c_void_p}
    return pointers, set(fields) - pointers


def test_search_families_name_the_librarys_symbols_and_structs():
    assert [fam.name for fam in K.ACO_FAMILIES] == ["aco_tsp", "aco_cvrp", "aco_prize"]
    assert sorted(env for fam in K.ACO_FAMILIES for env in fam.envs) == sorted(K.ACO_TD_KEYS)
    shared = {"B", "N", "n_ants", "iterations", "phases", "has_best", "alpha", "beta", "decay", "Q", "temperature", "reserved0",
              "philox_seed", "philox_offset"}
    for fam in K.ACO_FAMILIES:
        restype, argtypes = _lib.SYMBOLS[fam.symbol]
        assert argtypes[0] is ctypes.POINTER(fam.args) and restype is ctypes.c_int
        assert fam.symbol + "_lds_nodes" in _lib.SYMBOLS
        pointers, scalars = _pointers_and_scalars(fam.args)
        assert scalars == shared | set(fam.scalars)  # every scalar field has a value: none is left to the struct's zero
        keywords = set(inspect.signature(getattr(K, fam.name)).parameters)
        filled = {it.key for it in fam.instance} | {"pheromone", "log_heuristic", "ln_noise", "philox_seed_dev", "forced_actions",
                                                    "actions", "reward", "final_reward", "final_actions", "err"}
        filled |= {"start_nodes"} if fam.start_nodes else set()
        filled |= {"final_iteration"} if fam.ragged else set()
        assert filled <= pointers and filled <= keywords
        outputs = {"logps", "all_logps", "iter_actions", "iter_reward", "final_reward_cache", "logits_scratch"}
        outputs |= {"lengths", "iter_lengths"} if fam.ragged else set()
        assert pointers == filled | outputs
        assert ("start_nodes" in pointers) == fam.start_nodes and ("lengths" in pointers) == fam.ragged
        assert set(fam.cpu_refused) <= filled
        for env in fam.envs:  # the td mapping names keywords of the binding that serves the environment
            assert {kw for kw, _ in K.ACO_TD_KEYS[env]} <= {it.key for it in fam.instance}
            needed = [it.key for it in fam.instance if it.sample is True or (it.sample and env in it.sample)]
            assert set(needed) - {"locs"} == {kw for kw, _ in K.ACO_TD_KEYS[env]}


def test_gradient_families_name_the_librarys_symbols_and_structs():
    assert [fam.name for fam in K.ACO_GRAD_FAMILIES] == ["aco_tsp_logp_grad", "aco_depot_logp_grad"]
    assert sorted(env for fam in K.ACO_GRAD_FAMILIES for env in fam.envs) == sorted(K.ACO_TD_KEYS)
    for fam in K.ACO_GRAD_FAMILIES:
        restype, argtypes = _lib.SYMBOLS[fam.symbol]
        assert argtypes[0] is ctypes.POINTER(fam.args) and restype is ctypes.c_int
        pointers, scalars = _pointers_and_scalars(fam.args)
        assert scalars == {"B", "N", "n_ants", "row_split", "temperature", "reserved0"} | ({"env", "multistart"} if fam.depot else set())
        needs = {name for env in fam.envs for name, _ in fam.needs[env]}
        keywords = set(inspect.signature(getattr(K, fam.name)).parameters)
        assert needs <= keywords and set(fam.needs) == set(fam.envs)
        assert pointers == {"heatmap", "actions", "grad_ll", "grad_steps", "grad_heatmap", "err", fam.scratch[0]} | needs
        for env in fam.envs:  # what the backward takes is what the forward was given: locs or a td keyword
            assert {name for name, _ in fam.needs[env]} <= {"locs"} | {kw for kw, _ in K.ACO_TD_KEYS[env]}
    assert K.aco_family("spctsp").name == "aco_prize" and K.aco_grad_family("cvrp").name == "aco_depot_logp_grad"
