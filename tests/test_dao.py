"""DataDAO id-mapper and the compact->binary rewrite: the product's C++ (through the C ABI) against
(1) hand-derived expectations on the reference's own sample file, (2) the independent Python restatement,
bit-exact (integers and strings)."""
import os
import random

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from carskit_amd import dao
from oracle import dao_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def assert_same(d, o):
    assert d.raw_ids("user") == o["users"] and d.raw_ids("item") == o["items"]
    assert d.raw_ids("ui") == o["uis"] and d.raw_ids("ctx") == o["ctxs"]
    assert d.raw_ids("cond") == o["conds"] and d.raw_ids("dim") == o["dims"]
    assert d.cond_dim.tolist() == o["cond_dim"] and d.empty_context_conditions == o["empty"]
    assert d.ui_user.tolist() == o["ui_user"] and d.ui_item.tolist() == o["ui_item"]
    assert [d.ctx_conds[d.ctx_ptr[c]:d.ctx_ptr[c + 1]].tolist() for c in range(d.num_contexts)] == o["ctx_conds"]
    assert d.num_ratings == o["num_ratings"] and d.rating_scale == o["scale"]
    assert d.ui.tolist() == o["ui"] and d.ctx.tolist() == o["ctx"] and d.r.tolist() == o["r"]


def test_sample_train_binary_hand_derived():
    """Expectations derived by hand from DataDAO.readData on the reference's sampleData/train_binary.csv
    (SURVEY.md 8c-iv)."""
    d = dao.DataDAO(os.path.join(GOLDEN, "train_binary.csv"))
    assert (d.num_ratings, d.num_users, d.num_items, d.num_user_items, d.num_contexts, d.num_conditions,
            d.num_context_dims) == (20, 17, 2, 18, 8, 10, 3)
    assert d.empty_context_conditions == [2, 6, 7]
    assert d.raw_ids("user")[:4] == ["1077", "1052", "1070", "1045"]
    assert d.raw_ids("item") == ["tt0088763", "tt0120338"]
    assert d.raw_ids("ctx")[:5] == ["0,5,9", "0,5,8", "1,4,9", "1,5,9", "0,4,8"]
    assert list(zip(d.ui.tolist(), d.ctx.tolist(), d.r.tolist()))[:6] == [
        (0, 0, 4.0), (1, 1, 5.0), (2, 2, 5.0), (2, 3, 5.0), (3, 3, 4.0), (4, 4, 5.0)]
    assert d.r.sum() / np.count_nonzero(d.r) == 3.95
    assert d.raw_ids("dim") == ["companion", "location", "time"]
    assert d.cond_dim.tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert_same(d, dao_oracle.read_data(os.path.join(GOLDEN, "train_binary.csv")))
    rd = d.rating_data()
    assert rd.n == 20 and rd.u[:3].tolist() == [0, 1, 2] and rd.min_rate == 1.0 and rd.max_rate == 5.0


def test_sample_test_binary_matches_oracle():
    p = os.path.join(GOLDEN, "test_binary.csv")
    assert_same(dao.DataDAO(p), dao_oracle.read_data(p))


def _write_random_binary(path, rng, n_lines, n_users, n_items, dims, messy):
    conds = [(d, c) for d, k in enumerate(dims) for c in range(k)]
    sep = ",\t" if messy else ","
    hdr = ["User", " Item", " Rating"] + [" dim%d:%s" % (d, "na" if c == 0 else "c%d" % c) for d, c in conds]
    lines = [sep.join(hdr) + ("  " if messy else "")]
    for _ in range(n_lines):
        u = "u%d" % rng.randrange(n_users)
        i = "i%d" % rng.randrange(n_items)
        if messy and rng.random() < 0.2:
            u = u + " "                      # user keys are NOT trimmed individually
        r = rng.choice(["1", "2", "3.5", "4", "5", "0", " 2 ", "4.0d", "1e0"]) if messy else str(rng.randrange(1, 6))
        bits = []
        for d, k in enumerate(dims):
            on = rng.randrange(k) if (not messy or rng.random() < 0.9) else -1   # messy: sometimes no active condition
            bits += [(" 1" if messy else "1") if c == on else "0" for c in range(k)]
        lines.append("%s%s,%s,%s%s" % ("  " if messy else "", u, i, r, "".join("," + b for b in bits)))
    open(path, "w", newline="").write(("\r\n" if messy else "\n").join(lines) + ("" if messy else "\n"))


@settings(max_examples=30, deadline=None)
@given(seed=st.integers(0, 10_000), messy=st.booleans())
def test_dao_matches_oracle_on_random_files(tmp_path_factory, seed, messy):
    rng = random.Random(seed)
    p = str(tmp_path_factory.mktemp("dao") / "r.csv")
    _write_random_binary(p, rng, rng.randrange(1, 60), rng.randrange(1, 8), rng.randrange(1, 6),
                         [rng.randrange(1, 4) for _ in range(rng.randrange(0, 4))], messy)
    assert_same(dao.DataDAO(p), dao_oracle.read_data(p))


@pytest.mark.parametrize("threads", ["2", "5", "16"])
def test_dao_ranged_reader_matches_oracle_and_the_sequential_reader(tmp_path, threads, monkeypatch):
    """Files of 2^16 lines and more are parsed in ranges of lines on the host's cores (data_dao.cpp: per-range key tables, entered into
    the shared tables range after range).  Forced here on small random files -- many duplicate cells (the last line wins), keys first
    seen in any range, fewer lines than ranges, messy spacing -- and on a test file read over the training DAO's maps: the same ids,
    strings and matrix as the oracle and as the sequential reader, and the same error for a bad line in a late range."""
    monkeypatch.setenv("CMI_DAO_PARALLEL_MIN_LINES", "1")
    monkeypatch.setenv("CMI_HOST_THREADS", threads)
    rng = random.Random(int(threads))
    for case in range(12):
        p = str(tmp_path / ("r%d.csv" % case))
        _write_random_binary(p, rng, rng.choice([1, 3, 17, 400, 2500]), rng.randrange(1, 40), rng.randrange(1, 12),
                             [rng.randrange(1, 4) for _ in range(rng.randrange(0, 4))], messy=case % 3 == 0)
        assert_same(dao.DataDAO(p), dao_oracle.read_data(p))
    # `test-set`: the test DAO extends the training DAO's maps
    tr, te = str(tmp_path / "tr.csv"), str(tmp_path / "te.csv")
    _write_random_binary(tr, rng, 1500, 30, 9, [3, 2], messy=False)
    _write_random_binary(te, rng, 900, 45, 14, [3, 2], messy=False)
    d_tr = dao.DataDAO(tr)
    d_te = dao.DataDAO(te, train=d_tr)
    monkeypatch.setenv("CMI_DAO_PARALLEL_MIN_LINES", "1000000000")
    s_tr = dao.DataDAO(tr)
    s_te = dao.DataDAO(te, train=s_tr)
    for a, b in ((d_tr, s_tr), (d_te, s_te)):
        for kind in ("user", "item", "ui", "ctx", "cond", "dim"):
            assert a.raw_ids(kind) == b.raw_ids(kind), kind
        assert a.ui.tolist() == b.ui.tolist() and a.ctx.tolist() == b.ctx.tolist() and a.r.tolist() == b.r.tolist()
        assert a.ui_user.tolist() == b.ui_user.tolist() and a.ctx_conds.tolist() == b.ctx_conds.tolist() and a.rating_scale == b.rating_scale
        assert a.num_ratings == b.num_ratings
    # a bad line in the last range: the sequential pass reports it, with its line number
    monkeypatch.setenv("CMI_DAO_PARALLEL_MIN_LINES", "1")
    bad = str(tmp_path / "bad.csv")
    lines = open(tr).read().split("\n")
    f = lines[1200].split(",")
    f[2] = "abc"
    lines[1200] = ",".join(f)
    open(bad, "w").write("\n".join(lines))
    with pytest.raises(Exception) as ei:
        dao.DataDAO(bad)
    assert "line 1201" in str(ei.value) and "not a number" in str(ei.value)


def test_dao_errors():
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "bad.csv")
        open(p, "w").write("User,Item,Rating,a:x\nu,i,abc,1\n")
        with pytest.raises(Exception):
            dao.DataDAO(p)
        open(p, "w").write("User,Item,Rating,a:x\nu,i,3,\n")       # empty flag -> NumberFormatException
        with pytest.raises(Exception):
            dao.DataDAO(p)
        with pytest.raises(Exception):
            dao.DataDAO(os.path.join(td, "missing.csv"))


def test_java_hashmap_order_closed_form_equals_simulation():
    rng = random.Random(5)
    for n in (0, 1, 5, 12, 13, 24, 25, 100, 1000, 5043):
        keys = ["%d,tt%07d,%d,%s" % (rng.randrange(2000), rng.randrange(10 ** 7), rng.randrange(1, 6),
                                      rng.choice(["Weekend", "Weekday", ""])) + str(i) for i in range(n)]
        m = dao_oracle.JavaHashMap()
        for k in keys:
            m.put(k, 1)
        pos, tree = dao.java_hashmap_order(keys)
        assert [keys[i] for i in pos] == m.keys()
        assert tree == (m.max_bin >= 8 and n > 48) or not tree


def test_java_hashmap_order_ninth_node_of_a_small_bin_doubles_the_table():
    # String.hashCode of the nine first keys = 0 (mod 64): the ninth doubles the 16-slot table although 11 <= 12, so "aq" (3120) goes
    # to bucket 16 of 32 and "ab" (3105) to bucket 1
    keys = ["bb", "dd", "ff", "hh", "jj", "ll", "nn", "pp", "rr", "aq", "ab"]
    assert all(dao_oracle.jstring_hash(k) % 64 == 0 for k in keys[:9])
    want = keys[:9] + ["ab", "aq"]
    m = dao_oracle.JavaHashMap()
    for k in keys:
        m.put(k, 1)
    assert m.keys() == want and len(m.table) == 32
    pos, tree = dao.java_hashmap_order(keys)
    assert [keys[i] for i in pos] == want and not tree


def _short_keys(want, count, skip=0):
    """the short lower-case strings, shortest first, whose spread hash satisfies want(): `count` of them after the first `skip`"""
    import itertools
    import string
    out = []
    for n in (1, 2, 3):
        for t in itertools.product(string.ascii_lowercase, repeat=n):
            k = "".join(t)
            if want(dao_oracle.JavaHashMap._spread(k)):
                out.append(k)
                if len(out) == skip + count:
                    return out[skip:]
    raise AssertionError("not enough short keys")


def _simulated(keys):
    """the oracle's key order, and whether some put made a bin of 9 in a table of 64 slots or more at the time of that put"""
    m, tree = dao_oracle.JavaHashMap(), False
    for k in keys:
        slots = len(m.table) if m.table else 16
        m.put(k, 1)
        b = m._spread(k) & (slots - 1)
        tree |= slots >= 64 and sum((m._spread(q) & (slots - 1)) == b for q in m.keys()) >= 9
    return m.keys(), len(m.table), tree


def test_java_hashmap_tree_flag_is_decided_at_the_capacity_of_the_put():
    """30 keys bring the table to 64 slots; then nine keys share bin 5 of 64 (five in bin 5 of 128, four in bin 69), so the ninth
    makes a tree bin; 12 more keys double the table to 128 slots, where no bin holds more than five of them.  The flag must be set
    all the same.  Eight keys in bin 5 of 128 make no tree bin at either capacity: the flag must be clear."""
    head = _short_keys(lambda h: h % 64 != 5, 30)
    tail = _short_keys(lambda h: h % 64 != 5, 12, skip=30)
    nine = _short_keys(lambda h: h % 128 == 5, 5) + _short_keys(lambda h: h % 128 == 69, 4)
    eight = _short_keys(lambda h: h % 128 == 5, 8)
    for mid, want_tree in ((nine, True), (eight, False)):
        keys = head + mid + tail
        assert len(set(keys)) == len(keys)
        order, slots, sim_tree = _simulated(keys)
        assert slots == 128 and sim_tree == want_tree                 # the case is what it says
        pos, tree = dao.java_hashmap_order(keys)
        assert tree == want_tree
        assert [keys[i] for i in pos] == order


def test_java_string_hash_known_answers():
    # published String.hashCode values
    assert dao_oracle.jstring_hash("") == 0
    assert dao_oracle.jstring_hash("a") == 97
    assert dao_oracle.jstring_hash("hello") == 99162322
    assert dao_oracle.jstring_hash("Hello, World!") == (1498789909 & 0xFFFFFFFF)
    # "Aa" and "BB" collide (the classic example)
    assert dao_oracle.jstring_hash("Aa") == dao_oracle.jstring_hash("BB") == 2112


def test_compact_to_binary_sample(tmp_path):
    src = os.path.join(GOLDEN, "train_compact.csv")
    out = str(tmp_path / "train.csv")
    dao.transform_compact_to_binary(src, out)
    want, _ = dao_oracle.compact_to_binary(src)
    got = open(out).read().split("\n")
    assert got[-1] == "" and got[:-1] == want
    # the header the reference would write: dims in column order, conditions in first-seen order
    assert got[0].startswith("User, Item, Rating, ")
    # and the rewritten file loads through the DAO
    d = dao.DataDAO(out)
    assert d.num_ratings == len(want) - 1


@settings(max_examples=20, deadline=None)
@given(seed=st.integers(0, 10_000))
def test_compact_to_binary_random(tmp_path_factory, seed):
    rng = random.Random(seed)
    td = tmp_path_factory.mktemp("tr")
    src, out = str(td / "c.csv"), str(td / "b.csv")
    dims = ["Time", " Location", "Companion "][:rng.randrange(1, 4)]
    vals = [["Weekend", "Weekday", ""], ["Home", "Cinema", "NA"], ["Alone", "Family", "Partner", " friends"]]
    lines = ["userid,itemid,rating," + ",".join(dims)]
    for _ in range(rng.randrange(1, 200)):
        lines.append("%d,tt%05d,%d,%s" % (rng.randrange(50), rng.randrange(30), rng.randrange(1, 6),
                                        ",".join(rng.choice(vals[d]) for d in range(len(dims)))))
    open(src, "w").write("\n".join(lines) + "\n")
    dao.transform_compact_to_binary(src, out)
    want, _ = dao_oracle.compact_to_binary(src)
    assert open(out).read().split("\n")[:-1] == want


# ---- loose / binary input, merged (train + test) conditions, shared-map test DAO ------------------------------------

def _lines(path):
    return open(path).read().split("\n")[:-1]


@pytest.mark.parametrize("name,fmt", [("train_binary.csv", 1), ("train_loose.csv", 2), ("train_compact.csv", 3),
                                      ("test_binary.csv", 1), ("test_loose.csv", 2), ("test_compact.csv", 3)])
def test_validate_data_format_on_reference_samples(name, fmt):
    p = os.path.join(GOLDEN, name)
    assert dao.validate_data_format(p) == fmt
    assert dao_oracle.validate_format(dao_oracle.read_lines(p)) == fmt


@pytest.mark.parametrize("kind", ["loose", "compact", "binary"])
def test_transform_train_only(tmp_path, kind):
    src = os.path.join(GOLDEN, "train_%s.csv" % kind)
    out = str(tmp_path / "train.csv")
    dao.transform(src, out)
    want, _, _ = dao_oracle.transform(src)
    assert _lines(out) == want
    if kind == "binary":
        assert open(out, "rb").read() == open(src, "rb").read()       # copied verbatim
    d = dao.DataDAO(out)
    assert d.num_context_dims == 3
    ref = dao.DataDAO(os.path.join(GOLDEN, "train_binary.csv"))
    assert (d.num_users, d.num_items) == (ref.num_users, ref.num_items)
    if kind == "compact":
        # the compact sample describes the same 20 ratings as the binary sample (row order aside); the loose
        # format keys a rating by "user,item,rating", so same-valued ratings of a pair in different contexts merge
        assert d.nnz == ref.nnz and sorted(d.r.tolist()) == sorted(ref.r.tolist())


@pytest.mark.parametrize("tr,te", [("loose", "loose"), ("compact", "compact"), ("binary", "binary"),
                                   ("compact", "loose"), ("binary", "compact")])
def test_transform_with_test_set_and_shared_dao(tmp_path, tr, te):
    """`test-set` evaluation: conditions merged over both files (sorted, "na" added), both rewritten, and the test
    DAO extends the training DAO's id maps."""
    a, b = os.path.join(GOLDEN, "train_%s.csv" % tr), os.path.join(GOLDEN, "test_%s.csv" % te)
    oa, ob = str(tmp_path / "train.csv"), str(tmp_path / "test.csv")
    dao.transform(a, oa, b, ob)
    wa, wb, _ = dao_oracle.transform(a, b)
    assert _lines(oa) == wa and _lines(ob) == wb
    assert _lines(oa)[0] == _lines(ob)[0]                            # one header for both
    hdr = _lines(oa)[0].split(", ")[3:]
    assert hdr == sorted(hdr)                                        # TreeMultimap order
    assert all(any(h == d + ":na" for h in hdr) for d in {h.split(":")[0] for h in hdr})
    train = dao.DataDAO(oa)
    test = dao.DataDAO(ob, train=train)
    o = dao_oracle.read_data_shared(oa, ob)
    assert test.raw_ids("user") == o["users"] and test.raw_ids("item") == o["items"]
    assert test.raw_ids("ui") == o["uis"] and test.raw_ids("ctx") == o["ctxs"]
    assert test.ui_user.tolist() == o["ui_user"] and test.ui_item.tolist() == o["ui_item"]
    assert test.ui.tolist() == o["ui"] and test.ctx.tolist() == o["ctx"] and test.r.tolist() == o["r"]
    assert test.num_ratings == o["num_ratings"]
    assert test.raw_ids("user")[:train.num_users] == train.raw_ids("user")      # training ids are kept
    assert test.num_users >= train.num_users and test.num_contexts >= train.num_contexts


def test_shared_dao_rejects_a_different_header(tmp_path):
    a = os.path.join(GOLDEN, "train_binary.csv")
    train = dao.DataDAO(a)
    bad = tmp_path / "t.csv"
    bad.write_text("User,Item,Rating,x:a\nu,i,3,1\n")
    with pytest.raises(Exception):
        dao.DataDAO(str(bad), train=train)


@settings(max_examples=20, deadline=None)
@given(seed=st.integers(0, 10_000))
def test_transform_loose_random(tmp_path_factory, seed):
    rng = random.Random(seed)
    td = tmp_path_factory.mktemp("lo")
    src, out = str(td / "l.csv"), str(td / "b.csv")
    dims = {"Time": ["Weekend", "Weekday", ""], "Location": ["Home", "Cinema", "NA"], "Companion": ["Alone", "Family"]}
    lines = ["user,item,rating,dimension,condition"]
    for _ in range(rng.randrange(1, 60)):
        u, i, r = rng.randrange(8), rng.randrange(5), rng.randrange(1, 6)
        for d in rng.sample(list(dims), rng.randrange(1, 4)):
            lines.append("%d, tt%d ,%d,%s,%s" % (u, i, r, d, rng.choice(dims[d])))
    open(src, "w").write("\n".join(lines) + "\n")
    dao.transform(src, out)
    want, _, _ = dao_oracle.transform(src)
    assert _lines(out) == want
    dao.DataDAO(out)
