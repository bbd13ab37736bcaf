"""The parameter-server TCP edge is part of the boundary: its entry points are declared in
include/ono_reduce.h, exported by the library, bound by the Python mirror and by INTEGRATION.md's
Rust block with the header's arity, and counted by the docs.  CPU only."""
import re

import ono_amd
from ono_amd import _lib
from test_docs_abi import _read, header_decls, rust_bindings

NEW = {
    "ono_store_accumulate_sparse": 3, "ono_store_accumulate_sparse_dev": 3, "ono_sync_step_sparse": 6,
    "ono_push_settle_f32": 6,
    "ono_server_task_create": 5, "ono_server_task_run": 1, "ono_server_task_abort": 1, "ono_server_task_destroy": 1,
    "ono_cluster_create": 6, "ono_cluster_set_sparse": 3, "ono_cluster_set_sampler": 4, "ono_cluster_params": 2,
    "ono_cluster_grad": 2, "ono_cluster_residual": 2, "ono_cluster_size": 2, "ono_cluster_pull_params": 1,
    "ono_cluster_acc_residual": 2, "ono_cluster_push_grads": 2, "ono_cluster_abort": 1, "ono_cluster_destroy": 1,
}


def test_new_entry_points_are_declared_exported_and_bound():
    declared = ono_amd.header_functions()
    decls = header_decls()
    for name, arity in NEW.items():
        assert name in declared, f"{name} is not declared in include/ono_reduce.h"
        assert decls[name] == arity, f"{name}: {decls[name]} parameters in the header"
        assert hasattr(ono_amd.lib(), name), f"libono_reduce.so does not export {name}"
        assert name in _lib._SIGS and len(_lib._SIGS[name][1]) == arity, f"{name}: ono_amd._lib._SIGS"


def test_python_mirror_has_the_new_surface():
    assert callable(ono_amd.BlockingStore.accumulate_sparse) and callable(ono_amd.WildStore.accumulate_sparse)
    assert callable(ono_amd.BarrierSync.step_sparse) and callable(ono_amd.NoBlockingSync.step_sparse)
    assert callable(ono_amd.kernels.push_settle)
    for cls, methods in ((ono_amd.ServerTask, ("run", "abort", "close")),
                         (ono_amd.ServerClusterManager, ("set_sparse", "set_sampler", "pull_params", "acc_residual",
                                                         "push_grads", "abort", "close"))):
        for m in methods:
            assert callable(getattr(cls, m)), f"{cls.__name__}.{m}"


def test_rust_bindings_cover_the_new_entry_points():
    bound = {n: a for n, a, _ in rust_bindings()}
    for name, arity in NEW.items():
        assert bound.get(name) == arity, f"INTEGRATION.md: {name} bound with {bound.get(name)} parameters, header {arity}"


def test_docs_count_the_new_entry_points():
    n = len(header_decls())
    assert n == len(ono_amd.header_functions())
    for doc, pat in (("INTEGRATION.md", r"emits all (\d+) entry points"), ("README.md", r"C ABI \((\d+) entry points\)"),
                     ("DESIGN.md", r"C ABI, (\d+) entry points")):
        found = re.findall(pat, _read(doc))
        assert found and all(int(x) == n for x in found), f"{doc} quotes {found}, the header declares {n}"
    design = _read("DESIGN.md")
    assert "ono_store_accumulate_sparse" in design and "ono_sync_step_sparse" in design
    assert "ServerClusterManager" in _read("README.md")
