"""The L2 metric of the flat index, the parts that need no GPU:

* the float64 restatement (tests/l2_ref.py) has the contract's own properties: ascending, ties to the smaller id, pads (+inf, -1),
  exact zero for a query equal to a row, `id_base`, eligibility;
* the bias split (`vodhip_debug_l2_split`, vod_amd/csrc/l2_bias.h) for both store dtypes, over every half-integer up to 2^16, powers of
  two and their float32 neighbours up to the limit, and 10^5 seeded random values: sum_i const_i * term_i is within the stated
  residual r(c) of c (fp16: 2^-28, bf16: 2^-126), exact for every half-integer below 2^21, no term and no constant is subnormal in the
  store dtype, and |c| above the limit saturates (the bias stays at the limit, the call reports it);
* the factory accepts metric "l2" for a Flat index, names its store differently from inner_product, hands the metric to the server's
  command line, and still refuses other metrics and the sharded engines;
* the Gaussian seeds of tests/test_l2_gpu.py: the float32 FORM of the distance evaluated by NumPy orders fewer than 1 % of the top-100
  slots differently from the float64 restatement, so the GPU test's 1 % cap on id differences is one these seeds can meet.
"""
import ctypes

import numpy as np
import pytest

import l2_ref as R


def _split(values, dtype):
    from vod_amd import _native

    lib = _native.load_library()
    t = (ctypes.c_uint16 * 3)()
    a = (ctypes.c_float * 3)()
    terms = np.empty((len(values), 3), dtype=np.uint16)
    sat = np.empty(len(values), dtype=np.int64)
    consts = None
    for i, c in enumerate(values):
        sat[i] = lib.vodhip_debug_l2_split(ctypes.c_float(float(c)), dtype, t, a)
        terms[i] = t[:]
        consts = np.array(a[:], dtype=np.float64)
    return terms, consts, sat


def _reconstruct(terms, consts, dtype):
    return (R.term_value(terms, dtype) * consts[None, :]).sum(axis=1)  # float64: exact (three products of <= 24 bits)


def _sweep():
    rng = np.random.default_rng(20260219)
    half = -np.arange(0, 2 ** 17 + 1, dtype=np.float64) / 2          # every half-integer up to 2^16
    pow2 = []
    for e in range(-40, 24):                                          # powers of two and their float32 neighbours, below both limits
        p = np.float32(2.0 ** e)
        pow2 += [p, np.nextafter(p, np.float32(0)), np.nextafter(p, np.float32(np.inf))]
    rand = np.exp2(rng.uniform(-34, 23.9, size=100_000))              # log-uniform magnitudes: every binade gets its share
    wide_half = rng.integers(0, 2 ** 22, size=20_000) / 2             # half-integers up to 2^21
    return np.concatenate([half, -np.asarray(pow2, dtype=np.float64), -rand, -wide_half]).astype(np.float32)


@pytest.mark.parametrize("dtype", [R.F16, R.BF16], ids=["f16", "bf16"])
def test_split_reconstructs_c_within_the_stated_residual(dtype):
    c = _sweep()
    terms, consts, sat = _split(c, dtype)
    assert not sat.any()
    err = np.abs(_reconstruct(terms, consts, dtype) - c.astype(np.float64))
    assert err.max() <= R.RESIDUAL[dtype], (err.max(), c[err.argmax()])
    is_half = (c.astype(np.float64) * 2 == np.round(c.astype(np.float64) * 2)) & (np.abs(c) < 2 ** 21)
    assert is_half.sum() > 100_000 and err[is_half].max() == 0.0      # exact for half-integers below 2^21
    # the aim: within one float32 ulp of c wherever that ulp is not below the residual floor
    big = np.abs(c) >= 2.0 ** -5
    assert (err[big] <= np.spacing(np.abs(c[big])).astype(np.float64)).all()
    assert not R.is_subnormal(terms, dtype).any()
    # the query constants: powers of two, normal in the store dtype, and round-trip through it
    assert np.all(np.log2(consts) == np.round(np.log2(consts))) and consts.min() >= R.MIN_NORMAL[dtype]
    stored = consts.astype(np.float16).astype(np.float64) if dtype == R.F16 else R.round_store(consts, R.BF16)
    np.testing.assert_array_equal(stored, consts)


@pytest.mark.parametrize("dtype", [R.F16, R.BF16], ids=["f16", "bf16"])
def test_split_represents_norms_up_to_2_pow_23_and_saturates_above_the_limit(dtype):
    lim = np.float32(R.LIMIT[dtype])
    assert R.LIMIT[dtype] >= 2.0 ** 22                                # |x~|^2 = 2 |c| up to at least 2^23
    inside = -np.array([2.0 ** 22, 2.0 ** 22 + 0.5, lim, np.nextafter(lim, np.float32(0))], dtype=np.float32)
    terms, consts, sat = _split(inside, dtype)
    assert not sat.any()
    np.testing.assert_array_equal(_reconstruct(terms, consts, dtype), inside.astype(np.float64))
    outside = np.array([-np.nextafter(lim, np.float32(np.inf)), -lim * 2, -np.inf, np.nan, -3.0e38], dtype=np.float32)
    terms, consts, sat = _split(outside, dtype)
    assert (sat == 1).all()
    assert not R.is_subnormal(terms, dtype).any()
    np.testing.assert_array_equal(_reconstruct(terms, consts, dtype), np.full(len(outside), -float(lim)))  # ranks last, stays finite
    from vod_amd import _native

    t, a = (ctypes.c_uint16 * 3)(), (ctypes.c_float * 3)()
    assert _native.load_library().vodhip_debug_l2_split(ctypes.c_float(-1.0), 2, t, a) == -1  # float32 is no store dtype


def test_restatement_properties():
    rng = np.random.default_rng(5)
    x = rng.integers(-3, 4, size=(40, 7)).astype(np.float32)          # few values: many ties
    q = np.concatenate([x[[11, 3]], rng.integers(-3, 4, size=(6, 7)).astype(np.float32)])
    for dtype in (R.F16, R.BF16):
        d, i = R.l2_topk(q, x, 50, dtype, id_base=1000)
        assert d.shape == (8, 50) and i.dtype == np.int64
        assert (np.diff(d[:, :40], axis=1) >= 0).all()                # ascending
        tie = np.diff(d[:, :40], axis=1) == 0
        assert tie.any() and (np.diff(i[:, :40], axis=1)[tie] > 0).all()  # ties -> smaller id
        assert np.isposinf(d[:, 40:]).all() and (i[:, 40:] == -1).all()   # pads
        assert (np.sort(i[:, :40], axis=1) == np.arange(1000, 1040)).all()
        assert d[0, 0] == 0.0 and d[1, 0] == 0.0 and (d >= 0).all()   # a query equal to a row
        brute = ((q[:, None, :].astype(np.float64) - x[None].astype(np.float64)) ** 2).sum(-1)
        np.testing.assert_array_equal(np.sort(brute, axis=1), d[:, :40])
        elig = rng.random((8, 40)) < 0.3
        de, ie = R.l2_topk(q, x, 5, dtype, eligible=elig)
        for a in range(8):
            got = ie[a][ie[a] >= 0]
            assert elig[a, got].all() and len(got) == min(5, elig[a].sum())
    # rounding: the distance is that of the ROUNDED values
    xr = np.array([[1.0 + 2.0 ** -12, 0.0]], dtype=np.float32)
    d, _ = R.l2_topk(np.array([[1.0, 0.0]], dtype=np.float32), xr, 1, R.F16)
    assert d[0, 0] == 0.0
    d, i = R.l2_topk(np.zeros((2, 2), np.float32), np.zeros((0, 2), np.float32), 3, R.F16)
    assert np.isposinf(d).all() and (i == -1).all()


def test_factory_accepts_l2_and_refuses_the_rest(tmp_path):
    from vod_amd import factory

    x = np.random.default_rng(1).normal(size=(200, 16)).astype(np.float32)
    ip = factory.build_hip_mips_index(x, config={"port": 23470}, cache_dir=tmp_path)
    l2 = factory.build_hip_mips_index(x, config={"port": 23471, "metric": "l2"}, cache_dir=tmp_path)
    assert factory.HipMipsFactoryConfig(metric="l2").fingerprint() != factory.HipMipsFactoryConfig().fingerprint()
    assert l2.vectors_path != ip.vectors_path and l2.vectors_path.exists()
    cmd = l2._make_cmd()
    assert cmd[cmd.index("--metric") + 1] == "l2" and "--exact-f32" not in cmd   # float32 vectors: no float32 plane under L2
    assert "--metric" not in ip._make_cmd()
    for bad in ({"metric": "cosine"}, {"metric": "l1"}, {"factory": "IVF100,Flat", "metric": "l2"}, {"metric": "l2", "exact_f32": True}):
        with pytest.raises(ValueError):
            factory.build_hip_mips_index(x, config=bad, cache_dir=tmp_path)
    with pytest.raises(ValueError, match="single-device"):
        factory.build_hip_mips_index(x, config={"metric": "l2"}, cache_dir=tmp_path, devices=[0, 1])
    from vod_amd.search import server

    assert server.parse_args(["--vectors-path", "v.npy", "--metric", "l2"]).metric == "l2"
    with pytest.raises(SystemExit, match="single-device"):            # the node and group engines refuse at start-up, before any ingest
        server.main(["--vectors-path", "v.npy", "--metric", "l2", "--devices", "0,1", "--group-backend", "node"])
    with pytest.raises(SystemExit, match="single-device"):
        server.main(["--vectors-path", "v.npy", "--metric", "l2", "--devices", "0,1"])


GAUSS_CASES = [(768, "float16", 11), (768, "bfloat16", 12), (765, "float16", 13), (765, "bfloat16", 14)]  # shared with test_l2_gpu.py


def gauss_case(dim, seed, n=3000, nq=129):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, dim)).astype(np.float32), rng.standard_normal((n, dim)).astype(np.float32)


@pytest.mark.parametrize("dim,dtype,seed", GAUSS_CASES)
def test_gaussian_seeds_leave_float32_under_the_one_percent_cap(dim, dtype, seed):
    q, x = gauss_case(dim, seed)
    d64 = R.distances(q, x, dtype)
    _, ref_i = R.topk_from(d64, 100)
    _, emu_i = R.topk_from(R.float32_emulation(q, x, dtype).astype(np.float64), 100)
    differing = (ref_i != emu_i).mean()
    print(f"dim {dim} {dtype}: {100 * differing:.3f} % of the top-100 slots differ between float32 and float64")
    assert differing < 0.01
    # and the derived bound covers the float32 evaluation's own error everywhere
    assert (np.abs(R.float32_emulation(q, x, dtype).astype(np.float64) - d64) <= R.device_bound(q, x, dtype, d64)).all()
