"""The tensor half of tests/tools/mint_reference_cptf.py: DataDAO.toSparseTensor executed from DataDAO.java's source, and
TensorRecommender's fold split (TensorRecommender.java:66-83) over librec's SparseTensor executed from the jar's BYTECODE (clone,
getIndices, keys, value, set, remove, findIndex, buildIndex, the iterator).

Stand-ins added here, and the JDK / guava behaviour they assume (neither is part of the interpreted sources):
  * HashMultimap.create() -> HashSetMultimap below: guava 18's HashMultimap keeps a java.util.HashSet per key made by
    Sets.newHashSetWithExpectedSize(2) = new HashSet(3), a table of 4 slots.  The set iterates by bucket ((h ^ h >>> 16) & (slots - 1),
    h = the Integer's value), inside a bucket by insertion, and doubles when its size passes 3/4 of its slots (JDK 8 HashMap; a bin of
    8 keys is refused, as javasrc.JHashMap refuses it).  put, get, clear, putAll.
  * java.util.ArrayList (interp.JCollection) gains remove(int) (the element at the index, by descriptor `(I)`), set(int, E) and
    ArrayList(Collection) copying in iteration order.
  * the constructor of TensorRecommender cannot be called apart from Recommender's (configuration, static data): its loop, lines
    66-83, is driven statement for statement from Python over the bytecode's SparseTensor.  getKeys (:189-205) runs from source."""
import os

from oracle.jvm import interp, javasrc
from oracle.jvm.interp import VM, Box, JArray, JCollection
from oracle.mint_reference_src import sparse

ST = "librec/data/SparseTensor"


def _slots_order(keys):
    cap = 4
    for n in range(1, len(keys) + 1):
        if n > cap * 3 // 4:
            cap *= 2
    bins = {}
    for k in keys:
        h = int(k.v) & 0xFFFFFFFF
        bins.setdefault((h ^ (h >> 16)) & (cap - 1), []).append(k)
    if any(len(b) >= 8 for b in bins.values()):
        raise RuntimeError("a HashSet bin of 8 keys: tree bins are not simulated")
    return [k for b in sorted(bins) for k in bins[b]]


class HashSetMultimap:
    JAVA_TYPES = ("com/google/common/collect/Multimap",)

    def __init__(self):
        self.d = {}

    def jcall(self, vm, name, desc, args):
        if name == "put":
            s = self.d.setdefault(args[0], [])
            if args[1] in s:
                return 0
            s.append(args[1])
            return 1
        if name == "get":
            return JCollection(_slots_order(self.d.get(args[0], [])))
        if name == "clear":
            self.d.clear()
            return None
        if name == "putAll":              # Multimap.putAll(Multimap): entries() of the source, key by key in each set's iteration order
            changed = 0
            for k, vals in args[0].d.items():
                for v in _slots_order(vals):
                    changed |= self.jcall(vm, "put", "", [k, v])
            return changed
        if name == "size":
            return sum(len(v) for v in self.d.values())
        raise KeyError("HashMultimap." + name)


_jcollection_jcall = JCollection.jcall


def _jcollection_with_list_ops(self, vm, name, desc, args):
    if name == "remove" and desc.startswith("(I)"):
        return self.items.pop(int(args[0]))
    if name == "set":
        i = int(args[0].v if isinstance(args[0], Box) else args[0])
        old, self.items[i] = self.items[i], args[1]
        return old
    return _jcollection_jcall(self, vm, name, desc, args)


def install():
    JCollection.jcall = _jcollection_with_list_ops
    interp.HOST_STATICS[("com/google/common/collect/HashMultimap", "create")] = lambda vm: HashSetMultimap()


def new_vm(ref):
    return VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])


def boxed_map(d):
    m = javasrc.JHashMap()
    for k, v in d.items():
        m.d[Box(int(k), "Integer")] = v
    return m


def build_tensor(ref, n_pairs, n_ctx, cells, pair_user, pair_item, ctx_conds, cond_dim):
    """DataDAO.toSparseTensor(rateMatrix) from source.  Returns (vm, dao, tensor)"""
    install()
    vm = new_vm(ref)
    dao = javasrc.This(vm, [os.path.join(ref, "src", "carskit", "data", "processor", "DataDAO.java")],
                       {"SparseTensor": ST, "SparseMatrix": "librec/data/SparseMatrix"})
    dao.fields.update({"uiUserIds": boxed_map({p: Box(int(u), "Integer") for p, u in enumerate(pair_user)}),
                       "uiItemIds": boxed_map({p: Box(int(i), "Integer") for p, i in enumerate(pair_item)}),
                       "condDimensionMap": boxed_map({c: Box(int(d), "Integer") for c, d in cond_dim.items()}),
                       "contextConditionsList": boxed_map({c: JCollection([Box(int(x), "Integer") for x in conds])
                                                           for c, conds in enumerate(ctx_conds)}),
                       "dimensionConditionsList": None, "rateTensor": None,
                       "dimIds": JCollection(sorted(set(cond_dim.values())))})      # numContextDims() reads its size()
    rate_matrix = sparse(vm, n_pairs, n_ctx, cells)
    return vm, dao, dao.call("toSparseTensor", [rate_matrix])


def ints(x):
    if isinstance(x, JArray):
        return [int(v) for v in x.data]
    return [int(v.v if isinstance(v, Box) else v) for v in (x if isinstance(x, list) else x.items)]


def entries(vm, t):
    """the tensor in ITERATOR order: (keys, value) per TensorEntry"""
    out = []
    it = vm.invoke("virtual", ST, "iterator", "()Ljava/util/Iterator;", [t])
    while vm.invoke("interface", "java/util/Iterator", "hasNext", "()Z", [it]):
        te = vm.invoke("interface", "java/util/Iterator", "next", "()Ljava/lang/Object;", [it])
        keys = vm.invoke("interface", "librec/data/TensorEntry", "keys", "()[I", [te])
        out.append((ints(keys), float(vm.invoke("interface", "librec/data/TensorEntry", "get", "()D", [te]))))
    return out


def fold_split(vm, rate, pair_user, pair_item, test_cells):
    """TensorRecommender.java:66-83, statement for statement"""
    dims = vm.invoke("virtual", ST, "dimensions", "()[I", [rate])
    train = vm.invoke("virtual", ST, "clone", "()Llibrec/data/SparseTensor;", [rate])
    test = vm.new_object(ST)
    vm.call(ST, "<init>", "([I)V", [test, dims])
    vm.invoke("virtual", ST, "setUserDimension", "(I)V", [test, 0])
    vm.invoke("virtual", ST, "setItemDimension", "(I)V", [test, 1])
    for pair, _, _ in test_cells:
        u, i = int(pair_user[pair]), int(pair_item[pair])
        indices = vm.invoke("virtual", ST, "getIndices", "(II)Ljava/util/List;", [rate, u, i])
        for index in ints(indices):
            keys = vm.invoke("virtual", ST, "keys", "(I)[I", [rate, index])
            vm.invoke("virtual", ST, "set", "(D[I)V", [test, vm.invoke("virtual", ST, "value", "(I)D", [rate, index]), keys])
            vm.invoke("virtual", ST, "remove", "([I)Z", [train, keys])
    return train, test


def hexd(x):
    return float(x).hex()


def tensor_case(ref, name, n_users, n_items, ctx_dims, n_cells, n_test, seed, k=3):
    """one drawn rating matrix: the built tensor, getKeys of every context, one fold, predict(u, j, c) over a grid and evalRatings on
    a drawn model -- everything executed"""
    import numpy as np
    from mint_reference_cptf import new_this
    from oracle.mint_reference_src import dense
    rng = np.random.default_rng(seed)
    # conditions are numbered dimension by dimension; a context is one condition per dimension, in dimension order
    cond_dim, first = {}, []
    for d, n in enumerate(ctx_dims):
        first.append(len(cond_dim))
        for _ in range(n):
            cond_dim[len(cond_dim)] = d
    ctx_conds = sorted({tuple(first[d] + int(rng.integers(0, n)) for d, n in enumerate(ctx_dims)) for _ in range(12)}) or [()]
    ctx_conds = [list(c) for c in ctx_conds]
    pairs = sorted({(int(rng.integers(0, n_users)), int(rng.integers(0, n_items))) for _ in range(n_cells)})
    pair_user, pair_item = [p[0] for p in pairs], [p[1] for p in pairs]
    cellset = {}
    for _ in range(n_cells):
        cellset[(int(rng.integers(0, len(pairs))), int(rng.integers(0, len(ctx_conds))))] = float(rng.integers(1, 6))
    cells = [(p, c, v) for (p, c), v in sorted(cellset.items())]                     # rateMatrix order: rows, then columns
    test_cells = [cells[i] for i in sorted(rng.choice(len(cells), n_test, replace=False).tolist())]
    return executed_case(ref, name, n_users, n_items, pair_user, pair_item, ctx_conds, cond_dim, cells, test_cells, rng, k)


def executed_case(ref, name, n_users, n_items, pair_user, pair_item, ctx_conds, cond_dim, cells, test_cells, rng, k=3):
    from mint_reference_cptf import new_this
    from oracle.mint_reference_src import dense
    pairs = list(zip(pair_user, pair_item))
    rec = {"name": name, "n_users": n_users, "n_items": n_items, "pair_user": pair_user, "pair_item": pair_item,
           "ctx_conds": ctx_conds, "cond_dim": [cond_dim[c] for c in range(len(cond_dim))],
           "cells": [[p, c, hexd(v)] for p, c, v in cells], "test_cells": [[p, c, hexd(v)] for p, c, v in test_cells]}
    try:
        vm, dao, rate = build_tensor(ref, len(pairs), len(ctx_conds), cells, pair_user, pair_item, ctx_conds, cond_dim)
    except Exception as e:   # librec's SparseTensor refuses fewer than 3 dimensions
        rec["refused"] = repr(getattr(e, "args", [e])[0])[:200]
        return rec
    dims = ints(vm.invoke("virtual", ST, "dimensions", "()[I", [rate]))
    ents = entries(vm, rate)
    rec.update({"dims": dims, "keys": [x for ks, _ in ents for x in ks], "vals": [hexd(v) for _, v in ents],
                "dim_lists": {str(k_.v): ints(v) for k_, v in dao.fields["dimensionConditionsList"].d.items()}})
    train_t, test_t = fold_split(vm, rate, pair_user, pair_item, test_cells)
    train, test = entries(vm, train_t), entries(vm, test_t)
    rec.update({"train_keys": [x for ks, _ in train for x in ks], "train_vals": [hexd(v) for _, v in train],
                "test_keys": [x for ks, _ in test for x in ks], "test_vals": [hexd(v) for _, v in test]})
    # the model side: CPTF from source over these tensors
    _, this = new_this(ref)
    this.vm = vm
    M = [0.9 + 0.2 * rng.random((n, k)) for n in dims]
    dao.host["getDimensionConditionsList"] = lambda: dao.fields["dimensionConditionsList"]
    dao.host["getContextConditionsList"] = lambda: dao.fields["contextConditionsList"]
    this.fields.update({"M": [dense(vm, m) for m in M], "numDimensions": len(dims), "dimensions": JArray("I", dims), "userDimension": 0,
                        "itemDimension": 1, "numFactors": k, "rateDao": dao, "minRate": 1.0, "maxRate": 5.0, "view": "all",
                        "isResultsOut": False, "testTensor": test_t, "__enums__": ("Measure",)})
    ui = javasrc.JMap()
    for p_, (u_, i_) in enumerate(zip(pair_user, pair_item)):
        ui.d["%d,%d" % (u_, i_)] = Box(p_, "Integer")
    dao.fields["uiIds"] = ui
    rec["k"], rec["M"] = k, [hexd(x) for m in M for x in m.ravel()]
    rec["get_keys"] = [ints(this.call("getKeys", [0, 0, c]))[2:] for c in range(len(ctx_conds))]
    grid = [(u, j, c) for u in range(min(n_users, 2)) for j in range(min(n_items, 3)) for c in range(len(ctx_conds))]
    rec["predict_ujc"] = [[u, j, c, hexd(javasrc.unbox(this.call("predict", [u, j, c])))] for u, j, c in grid]
    measures = this.call("evalRatings", [])
    rec["eval_ratings"] = {key.name: hexd(javasrc.unbox(v)) for key, v in measures.d.items()}
    return rec
