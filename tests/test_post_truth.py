"""The CPU oracle's post chain (oracle/denoiser_oracle.cpp, post_oracle.cpp, tonemap of ptrt_oracle.cpp) against the float64 statement
of the reference in tests/post_truth.py: the measured table, the decided cap, the documented cases and the seeded misreadings
(DESIGN 5.4).  tests/test_post_truth_gpu.py holds the kernels to the same statement and to the oracle's bits."""
import numpy as np
import pytest

import post_truth as T


@pytest.fixture(scope="module")
def table(O):
    best, shares = T.measure(O)
    print("\nquantity   largest deviation (units)   attained by                     x 4 = TOL")
    for q in T.MEASURED:
        print(f"{q:10s} {best[q][0]:8.3f}                    {best[q][1]:30s} {4 * best[q][0]:.2f}")
    return best, shares


@pytest.fixture(scope="module")
def items():
    return T.ITEMS()


def test_the_oracle_fits_the_statement_and_the_table_is_what_it_measures(table):
    best, _ = table
    for q, (where, value) in T.MEASURED.items():
        assert best[q][0] <= T.TOL[q], f"{q}: {best[q][0]:.3f} units on {best[q][1]}, tolerance {T.TOL[q]:.3f}"
        assert abs(best[q][0] - value) <= 0.02 * value, f"{q}: {best[q][0]:.3f} on {best[q][1]}, table says {value} on {where}"
        assert best[q][1] == where, f"{q}: attained by {best[q][1]}, table says {where}"


def test_named_terms_are_worth_what_the_module_says(O):
    try:
        for term, name in sorted({(t, n) for t, n, _ in T.WITHOUT_TERMS}):
            T.NAMED_TERMS[term] = False
            best, _ = T.measure(O, names=(name,))
            T.NAMED_TERMS[term] = True
            for (t, n, q), value in T.WITHOUT_TERMS.items():
                if (t, n) == (term, name):
                    assert abs(best[q][0] - value) <= 0.02 * value, f"without {term}, {q} on {name}: {best[q][0]:.3f}, recorded {value}"
    finally:
        for term in T.NAMED_TERMS:
            T.NAMED_TERMS[term] = True


def test_decided_cap_from_the_statement_alone(table, items):
    _, shares = table
    worst = {}
    for key, und in shares.items():
        name = key.rsplit(" ", 1)[0]
        worst[name] = max(worst.get(name, 0.0), max(und.values()))
        if items[name].get("threshold"):
            continue
        for k, share in und.items():
            assert share <= T.MAX_UNDECIDED, f"{key}, k = {k}: {100 * share:.2f} % undecided"
    for name, share in worst.items():
        print(f"{name:32s} undecided, most of any (frame, k): {100 * share:.3f} %")
    for name, it in items.items():                                      # the items that sit ON a threshold say so and are undecided there
        if it.get("threshold"):
            assert worst[name] > 0.0, name


def test_atrous_iterations_are_clamped_to_0_and_5(O, items):
    """`mini(atrous_iters, 5)` and a loop a negative count never enters: 7 gives what 5 gives, -1 what 0 gives (the temporal image)."""
    assert T.atrous_passes(T.settings(atrous_iterations=7)) == 5 and T.atrous_passes(T.settings(atrous_iterations=-1)) == 0
    assert set(T.atrous_passes(T.settings(atrous_iterations=k)) for k in T.ATROUS_VARIANTS) == set(range(6))
    it = items["plain/65x17"]
    W, H = it["W"], it["H"]
    for r in T.oracle_frames(O, it, ks=(7, 5, -1, 0)):
        assert np.array_equal(r["outs"][7].view(np.uint32), r["outs"][5].view(np.uint32)), r["f"]
        assert np.array_equal(r["outs"][-1].view(np.uint32), r["outs"][0].view(np.uint32)), r["f"]
        assert T.deviation(r["outs"][7].reshape(H, W, 3), r["T"]["out"][5], r["T"]["decided"][5])[0] <= T.TOL["out5"]
        assert T.deviation(r["outs"][-1].reshape(H, W, 3), r["T"]["out"][0], r["T"]["decided"][0])[0] <= T.TOL["out0"]


def _statement_sequence(it, s, frames=None, mis=()):
    """The statement fed with its OWN history (float32-rounded, as a history is), for the cases asserted on the statement alone."""
    hist, out = None, []
    for fr in (frames or it["frames"]):
        H, W = fr["depth"].shape
        r = T.denoise_frame(s, hist, fr["color"], fr["normal"], fr["depth"], fr["obj"], np.zeros((H, W, 2), np.float32), mis)
        hist = dict(mean=r["hmean"].v.astype(np.float32).astype(np.float64), m2=r["hm2"].v.astype(np.float32).astype(np.float64),
                    len=r["hlen"].v.astype(np.float32).astype(np.float64), normal=fr["normal"], depth=fr["depth"], obj=fr["obj"])
        out.append(r)
    return out


def test_three_settings_are_ignored(items):
    """firefly_threshold, sigma_normal and sigma_depth reach the kernels and are never read (denoiser.cuh:416-419, :650-749)."""
    it = items["plain/65x17"]
    a = _statement_sequence(it, T.settings())
    b = _statement_sequence(it, T.settings(firefly_threshold=0.5, sigma_normal=1.0, sigma_depth=100.0))
    for ra, rb in zip(a, b):
        for k in range(6):
            assert np.array_equal(ra["out"][k].v, rb["out"][k].v)
    c = _statement_sequence(it, T.settings(sigma_luminance=0.5))        # (a setting that IS read does change the answer)
    assert not np.array_equal(a[0]["out"][1].v, c[0]["out"][1].v)


def test_constant_image_is_a_fixed_point():
    W, H = 33, 9
    fr = dict(color=np.full((H, W, 3), 0.25, np.float32), normal=np.broadcast_to(np.float32(T.N_UP), (H, W, 3)).copy(),
              depth=T.plane_depth(W, H, 4.0), obj=np.zeros((H, W), np.int32))
    for r in _statement_sequence(None, T.settings(), frames=[fr] * 3):
        for k in range(6):
            assert r["decided"][k].all()
            assert np.abs(r["out"][k].v - 0.25).max() <= 1e-12         # (the weights are renormalised: exact but for the division)
        assert np.abs(r["hm2"].v - 0.0625).max() <= 1e-12 and (r["hlen"].v[1:-1, 1:-1] > 1.0).all()


def test_self_rejecting_normal_passes_through_unfiltered(items):
    """0.1 <= |n|^2 < edge_normal_threshold: not sky, yet every comparison with itself fails the edge rule.  No 3x3 neighbour
    (the `neighbor_count == 0` branch, denoiser.cuh:490-494), no history tap and no a-trous tap is accepted: the history never
    grows and every pass returns the centre."""
    it = items["self_rejecting/65x17"]
    half = it["half"]
    assert half.sum() > 40 and (~half).sum() > 40
    for f, r in enumerate(_statement_sequence(it, it["settings"])):
        assert (r["ncount"][half] == 0).all() and (r["ncount"][~half] > 0).all()
        assert not r["valid"][half].any() and (r["hlen"].v[half] == 1.0).all()
        assert np.array_equal(r["hmean"].v[half], T.firefly(it["frames"][f]["color"].astype(np.float64), it["frames"][f]["depth"],
                                                              it["frames"][f]["normal"], it["settings"])[0].v[half])
        for k in range(1, 6):
            assert np.array_equal(r["out"][k].v[half], r["out"][0].v[half])
            assert r["decided"][k][half].all()
        assert not np.array_equal(r["out"][1].v[~half], r["out"][0].v[~half])


def test_history_length_after_static_frames():
    """init_moments sets 1 and the first frame accumulates onto it at once: 2, 3, ... up to max_history, where it stays."""
    W, H = 17, 5
    frames = [dict(color=T.colours(W, H, 900 + f, 0), normal=np.broadcast_to(np.float32(T.N_UP), (H, W, 3)).copy(),
                   depth=T.plane_depth(W, H, 4.0), obj=np.zeros((H, W), np.int32)) for f in range(6)]
    lens = [r["hlen"].v for r in _statement_sequence(None, T.settings(max_history=4.0), frames=frames)]
    inner = (slice(1, H - 1), slice(1, W - 1))                          # (prev_u >= W - 0.5 has no history in the last column and row)
    assert [float(np.unique(ln[inner])[0]) for ln in lens] == [2.0, 3.0, 4.0, 4.0, 4.0, 4.0]
    assert all(np.unique(ln[inner]).size == 1 for ln in lens)
    assert (lens[3][:, W - 1] == 1.0).all() and (lens[3][H - 1, :] == 1.0).all()


def test_items_reach_the_branches_they_are_built_for(O, items):
    """From the statement's own masks: taps that straddle a step (none valid -> `nearest`; exactly one valid) on the first frame
    and after it; only the centre of a 3x3 window on its surface; reprojection off screen; max_history reached."""
    for name in ("steps_creases/129x33",):
        rs = list(T.oracle_frames(O, items[name], ks=(0,)))
        for r in (rs[0], rs[1]):
            tv = r["T"]["taps_valid"]
            assert (tv == 0).sum() >= 1 and (tv == 1).sum() >= 1 and (tv == 4).sum() >= 1, (name, r["f"])
    r = next(T.oracle_frames(O, items["checker1/129x33"], ks=(0,)))
    assert (r["T"]["ncount"] == 1).sum() > 100
    rs = list(T.oracle_frames(O, items["plain/131x77"], ks=(0,)))
    assert not rs[2]["T"]["on"][:, :5].any() and rs[2]["T"]["on"][:60, 8:].all()
    rs = list(T.oracle_frames(O, items["plain_moved/131x77"], ks=(0,)))
    assert (rs[2]["T"]["hlen"].v == 3.0).sum() > 1000 and rs[2]["T"]["hlen"].v.max() == 3.0
    r = next(T.oracle_frames(O, items["plain/1x1"], ks=(0,)))            # 1x1: prev_u = 0.5 >= W - 0.5, and no firefly neighbour
    assert not r["T"]["on"].any() and np.array_equal(r["T"]["out"][5].v, items["plain/1x1"]["frames"][0]["color"].astype(np.float64))


# ------------------------------------------------------------------------------------------------ seeded misreadings
def _denoiser_caught(O, items, name, mis, quantities):
    it = items[name]
    W, H = it["W"], it["H"]
    for r in T.oracle_frames(O, it, mis=(mis,)):
        dev, _ = T.judge_frame(r, W, H)
        for q in quantities:
            if dev[q][0] > T.TOL[q]:
                return True
    return False


@pytest.mark.parametrize("mis,name,quantities", [
    ("atrous_kernel_1242", "plain/65x17", ("out1",)),
    ("luminance_rb", "plain/65x17", ("out1",)),
    ("boost_1", "plain_moved/131x77", ("out1",)),
    ("taps_12", "plain/65x17", ("hmean",)),
    ("alpha_1_over_len", "plain/65x17", ("hmean",)),
    ("clamp_never", "plain/65x17", ("hmean",)),
])
def test_seeded_misreadings_of_the_denoiser_are_caught(O, items, mis, name, quantities):
    assert not _denoiser_caught(O, items, name, "", quantities)
    assert _denoiser_caught(O, items, name, mis, quantities), mis


def test_soft_clamp_of_an_invalid_history_cannot_be_seen(O, items):
    """`clamp_invalid` (the soft clamp applied to an invalid history as well) changes NO output: an invalid history has alpha = 1,
    and out = hist * (1 - 1) + cur * 1 multiplies whatever hist holds by an exact 0 (denoiser.cuh:567-583).  It is kept among the
    seeded misreadings and asserted to be invisible; `clamp_never` (no clamp for a valid history either) is its visible neighbour."""
    it = items["plain/131x77"]
    for r, m in zip(T.oracle_frames(O, it, ks=(0,)), T.oracle_frames(O, it, ks=(0,), mis=("clamp_invalid",))):
        assert (~r["T"]["valid"]).sum() > 100 or r["f"] == 0
        for key in ("hmean", "hm2", "hlen"):
            assert np.array_equal(r["T"][key].v, m["T"][key].v), (key, r["f"])


@pytest.mark.parametrize("mis,size", [("knee_1", (64, 64)), ("up_true_size", (131, 77)), ("up_true_size", (65, 64))])
def test_seeded_misreadings_of_bloom_are_caught(O, mis, size):
    W, H = size
    img = T.bloom_images(W, H)["spots"]
    got = O.bloom(img, W, H)
    assert T.deviation(got, T.bloom(img, W, H))[0] <= T.TOL["bloom"]
    assert T.deviation(got, T.bloom(img, W, H, (mis,)))[0] > T.TOL["bloom"]


@pytest.mark.parametrize("mis", ["gamma_22", "scale_255"])
def test_seeded_misreadings_of_the_tonemap_are_caught(O, mis):
    img = np.random.RandomState(8).uniform(0, 1, (4096, 3)).astype(np.float32) ** 3 * 4.0
    val, byte, dec = T.tonemap(img)
    got = O.tonemap(img, 64, 64)[::-1].reshape(-1, 3).astype(np.int64)  # (the kernel writes row H - 1 - y)
    assert T.deviation(O.tonemap_float(img), val)[0] <= T.TOL["tonemap"]
    assert np.array_equal(got[dec], byte[dec]) and np.abs(got - byte).max() <= 1 and dec.mean() > 0.98
    mval, mbyte, mdec = T.tonemap(img, (mis,))
    if mis == "gamma_22":
        assert T.deviation(O.tonemap_float(img), mval)[0] > T.TOL["tonemap"]
    assert (got[mdec] != mbyte[mdec]).any()


def test_misreadings_are_the_ones_listed():
    assert set(T.MISREADINGS) == {"atrous_kernel_1242", "luminance_rb", "boost_1", "taps_12", "alpha_1_over_len", "clamp_invalid",
                                  "clamp_never", "knee_1", "up_true_size", "gamma_22", "scale_255"}


# ------------------------------------------------------------------------------------------------ bloom, up-scale, tonemap
def test_bloom_documented_cases(O):
    """A dim image gets no bloom; a constant image above the knee keeps its value through every level (the five taps sum to
    0.999999 in float32 weights), so the frame ends at about 7 x the constant; odd sizes leave the last row / column without."""
    W, H = 66, 65
    dim = np.full((H * W, 3), 0.45, np.float32)
    assert np.array_equal(T.bloom(dim, W, H).v, dim.astype(np.float64))
    assert np.allclose(T.bloom(np.full((64 * 64, 3), 2.5, np.float32), 64, 64).v, 7 * 2.5, rtol=1e-4)
    c = T.bloom(np.full((H * W, 3), 2.5, np.float32), W, H).v.reshape(H, W, 3)
    assert (c[:64] > 2.5).all() and np.array_equal(c[64], np.full((W, 3), 2.5))
    with pytest.raises(ValueError):
        T.bloom(np.zeros((32 * 32, 3), np.float32), 32, 32)


def test_rgb8_is_equal_on_decided_bytes_and_within_one_elsewhere(O):
    for (W, H) in ((66, 65), (131, 77)):
        img = O.bloom(T.bloom_images(W, H)["spots"], W, H)
        _, byte, dec = T.tonemap(img)
        got = O.tonemap(img, W, H)[::-1].reshape(-1, 3).astype(np.int64)
        assert np.array_equal(got[dec], byte[dec]), (W, H)
        assert np.abs(got - byte).max() <= 1 and dec.mean() > 0.97


def test_python_settings_mirror_the_c_struct(P, O):
    """ptrt_amd.DenoiserSettings: the fields of ptrt_denoiser_settings in order, filled by ptrt_denoiser_default_settings with the
    reference's diffuse_* defaults -- the statement's and the oracle's."""
    d = P.DenoiserSettings()
    assert tuple(n for n, _ in d._fields_) == T.FIELDS == tuple(n for n, _ in O.DenoiserSettings._fields_)
    o, s = O.DenoiserSettings(), T.settings()
    for k in T.FIELDS:
        assert getattr(d, k) == getattr(o, k) == s[k], k
    m = P.DenoiserSettings(**T.settings(**T.moved_settings()))
    assert m.max_history == 3.0 and m.atrous_iterations == 5 and abs(m.tau - 0.11) < 1e-7
    with pytest.raises(AttributeError):
        P.DenoiserSettings(sigma=1.0)
    with pytest.raises(TypeError):
        P.Scene(8, 8, device=P.HOST_ONLY).setDenoiserSettings(None)
