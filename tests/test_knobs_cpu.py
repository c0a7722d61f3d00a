"""CPU checks of what the environment-knob tests stand on (tests/_knobs.py): every knob the sources read is placed somewhere, every
case takes the branch it was written for under its group's environment and another one without it, the edges its comments claim
are arithmetic on its shape, the project's bar is fair to fp32 on every case, and a backward that recomputes its probabilities
in the other unit system than the forward formed them is outside the bar on the x6 inputs."""
import glob
import math
import os
import re

import pytest
import torch

from tests import _attn_bwd as AB
from tests import _knobs as K
from tests.test_switches_cpu import table_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "m-cedm_amd", "csrc")


def knobs_in_the_sources():
    found = set()
    for p in glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")):
        found |= set(re.findall(r'env_int\("(MCEDM_[A-Z0-9_]+)"', open(p).read()))
    return found


def test_every_knob_is_accounted_for():
    """A knob added later fails here until someone decides where it runs."""
    knobs = knobs_in_the_sources()
    switches = {env for _, env, _ in table_rows()}
    assert len(switches) == 10 and len(knobs) >= 15, (switches, knobs)
    grouped = set().union(*(env for env, _ in K.GROUPS.values()))
    places = {"GROUPS": grouped, "COVERED_ELSEWHERE": set(K.COVERED_ELSEWHERE), "EXCLUDED": set(K.EXCLUDED), "switches": switches}
    for name in sorted(knobs | switches):
        at = [p for p, s in places.items() if name in s]
        assert len(at) == 1, (name, at)
    for p, s in places.items():
        assert s <= knobs | switches, (p, s - knobs - switches)      # nothing placed that the sources no longer read
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    doc = doc[doc.index("## Environment switches"):]
    assert not [k for k in sorted(knobs | switches) if f"`{k}`" not in doc]


def test_the_named_tests_exist():
    named = list(K.COVERED_ELSEWHERE.values()) + [(f, t) for _, f, t in K.EXCLUDED.values() if f]
    assert len(named) == len(K.COVERED_ELSEWHERE) + 1
    for path, fn in named:
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(rf"^def {fn}\(", src, flags=re.M), (path, fn)
    for knob, (path, fn) in K.COVERED_ELSEWHERE.items():
        assert knob in open(os.path.join(ROOT, path)).read(), (knob, path)


def test_the_restated_predicates():
    assert [K.attn_fwd_row(T)[17:-1] for T in (64, 127, 128, 255, 256, 511, 512, 529, 1024)] == [
        "one", "one", "split<2>", "split<2>", "split<4>", "split<4>", "lds<2>", "split<4>", "lds<2>"]
    assert K.attn_fwd_row(512, aligned=False) == "attention_kernel[split<4>]"
    assert [K.attn_bwd_row(T) for T in (1, 64, 128, 129, 256)] == ["attention_bwd_" + AB.branch(T) for T in (1, 64, 128, 129, 256)]
    # the units the backward must take: the forward's
    assert [K.attn_fwd_base2(T) for T in (127, 128)] == [False, True]
    assert not any(K.attn_fwd_base2(T, {"MCEDM_ATTN_SPLIT": "0"}) for T in (128, 256, 1024))
    assert K.attn_fwd_base2(64, {"MCEDM_ATTN_LDS_MIN": "64"}) and not K.attn_fwd_base2(66, {"MCEDM_ATTN_LDS_MIN": "64"})


ATTN = [k for k, c in K.CASES.items() if c.kind.startswith("attn")]
GN = [k for k, c in K.CASES.items() if c.kind == "gn"]


def test_every_case_needs_its_child():
    """Under the group's environment the restated predicate gives the rows the case claims; under the default environment it
    does not (attn_xcd0 apart: that knob changes no row, only the order of the workgroups)."""
    for name, (env, keys) in K.GROUPS.items():
        assert keys and len(set(keys)) == len(keys), name
        for key in keys:
            c = K.CASES[key]
            assert not set(c.must) & set(c.must_not), key
            if c.kind.startswith("attn"):
                T = c.shape[2] * c.shape[3]
                want = (K.attn_fwd_row(T, env),) + ((K.attn_bwd_row(T, env),) if c.kind == "attn_pair" else ())
                dflt = (K.attn_fwd_row(T),) + ((K.attn_bwd_row(T),) if c.kind == "attn_pair" else ())
                assert set(c.must_not) == set(K.ATTN_ROWS) - set(want), key
            elif c.kind == "gn":
                want, dflt = (K.gn_bwd_row(c.shape, env),), (K.gn_bwd_row(c.shape),)
            elif c.kind == "wino":
                want, dflt = (K.wino_row(c.shape, env),), (K.wino_row(c.shape),)
            else:
                want, dflt = (K.c1_row(c.shape[3], env),), (K.c1_row(c.shape[3]),)
            assert c.must == want, (key, c.must, want)
            if name == "attn_xcd0":
                assert want == dflt and c.shape[0] * c.shape[1] % 8 == 0, key     # the remap is the identity unless B heads % 8 == 0
            elif key.startswith(("attn_lds1/fwd/T529/", "attn_ldsmin/fwd/T130/", "wino_min256/wino/2_64_0_64_8_16")):
                assert want == dflt, key                                            # the cases that must NOT take the group's kernel
            else:
                assert want != dflt, (key, want, dflt)


def test_the_attention_tables_reach_what_they_claim():
    def Ts(group, kind):
        return sorted({K.CASES[k].shape[2] * K.CASES[k].shape[3] for k in K.GROUPS[group][1] if K.CASES[k].kind == kind})
    for g in ("attn_split0", "attn_split2", "attn_lds1", "attn_ldsmin", "attn_ldsmin16", "attn_xcd0"):
        subs = {K.CASES[k].sub for k in K.GROUPS[g][1] if K.CASES[k].kind == "attn_fwd"}
        assert subs == {"plain", "spike", "x6"}, (g, subs)
    # attn_split0: 4 to 17 key tiles on one wave, a ragged last tile at 169 and 529; the pairs on direct<4> and on the LDS kernels
    assert Ts("attn_split0", "attn_fwd") == [128, 169, 256, 512, 529]
    assert [math.ceil(T / 32) for T in Ts("attn_split0", "attn_fwd")] == [4, 6, 8, 16, 17] and 169 % 32 and 529 % 32
    assert Ts("attn_split0", "attn_pair") == [129, 169, 256, 512]
    assert {K.attn_bwd_row(T) for T in (129, 169, 256, 512)} == {"attention_bwd_direct<4>", "attention_bwd_lds"}
    # attn_split2: key tiles per wave of split<4> (wave w takes tiles w, w + 4, ...): the merge of unequal counts at 576
    per_wave = {T: [len(range(w, math.ceil(T / 32), 4)) for w in range(4)] for T in Ts("attn_split2", "attn_fwd")}
    assert per_wave == {512: [4, 4, 4, 4], 576: [5, 5, 4, 4], 640: [5, 5, 5, 5]}
    assert Ts("attn_split2", "attn_pair") == [128, 256, 384, 512]
    assert all(K.attn_bwd_row(T) == "attention_bwd_lds" for T in (128, 256, 384, 512))        # ... which the default sends to the LDS kernels
    # attn_lds1: 32-key staged tiles; 516: 4 keys in the last one and 4 queries in the last workgroup's first tile, the other three empty
    assert Ts("attn_lds1", "attn_fwd") == [512, 516, 529, 544, 640]
    assert 516 % 32 == 4 and 516 % 128 == 4 and 544 % 32 == 0 and 544 % 128 == 32 and 529 % 4
    # attn_ldsmin: 64-key staged tiles, waves 4..7 on the odd 32 keys of each
    staged = {T: math.ceil(T / 64) for T in Ts("attn_ldsmin", "attn_fwd") if T != 130}
    assert staged == {128: 2, 132: 3, 160: 3, 192: 3, 256: 4} and max(staged.values()) < 8
    for T in (132, 160):          # the odd half of the last staged tile lies wholly past T, the even half does not
        k0 = 64 * (staged[T] - 1)
        assert k0 < T <= k0 + 32, T
    assert all(64 * (staged[T] - 1) + 32 < T for T in (128, 192, 256))
    assert 130 % 4 and K.attn_fwd_row(130, K.GROUPS["attn_ldsmin"][0]) == "attention_kernel[split<2>]"
    assert Ts("attn_ldsmin", "attn_pair") == [132, 256]


def test_the_one_tile_and_winograd_tables_reach_what_they_claim():
    # attn_ldsmin16: ONE staged tile of 64 keys whose odd half [32, 64) lies wholly past T: waves 4..7 never see a key
    env = K.GROUPS["attn_ldsmin16"][0]
    Ts = sorted(K.LDSMIN16_SHAPE)
    assert Ts == [16, 20, 32] and all(math.ceil(T / 64) == 1 and T <= 32 and T % 4 == 0 for T in Ts) and 20 % 32 and 32 % 32 == 0
    assert all(K.attn_fwd_row(T, env) == "attention_kernel[lds<2>]" and K.attn_fwd_row(T) == "attention_kernel[one]" for T in Ts)
    assert K.attn_bwd_row(32, env) == "attention_bwd_direct<1>" and K.attn_fwd_base2(32, env) and not K.attn_fwd_base2(32)
    # wino_min256: whole 8 x 16 tiles, 64- and 128-channel outputs (WinoCfg<2>, WinoCfg<4>), two sources, two tile columns
    env = K.GROUPS["wino_min256"][0]
    assert all(s[4] % 8 == 0 and s[5] % 16 == 0 and s[3] % 64 == 0 and s[1] % 8 == 0 and (s[1] + s[2]) % 8 == 0 for s in K.WINO_CASES)
    large = [s for s in K.WINO_CASES if K.wino_row(s, env) == K.WINO_LARGE]
    assert sorted(s[4] * s[5] for s in large) == [256, 256, 512] and {s[3] for s in large} == {64, 128} and any(s[2] for s in large)
    assert all(K.wino_row(s) == K.WINO_SPLIT for s in K.WINO_CASES)                # the default sends every one to the split form
    assert [s for s in K.WINO_CASES if s not in large] == [(2, 64, 0, 64, 8, 16)]


def test_the_groupnorm_table_reaches_what_it_claims():
    forms = sorted(K.gn_reg_quads(c) for c in K.GN_CASES if K.gn_reg_quads(c)[0])
    assert forms == [(1, 16), (1, 64), (2, 64), (4, 64), (8, 64)], forms
    lds = [c for c in K.GN_CASES if K.gn_lds_served(c)]
    assert [c[5] for c in lds] == [0, 1, 2] and all(c[3] * c[4] == 4096 for c in lds)
    C = lds[0][1] + lds[0][2]
    assert C // K.gn_groups(C) * 4096 == 16384                      # the smallest slab the LDS-resident kernel takes
    assert all(K.gn_lds_served(c) or K.gn_reg_quads(c)[0] for c in K.GN_CASES)
    rows = {g: [K.CASES[k].must[0] for k in K.GROUPS[g][1]] for g in ("gn_twopass256", "gn_twopass1024")}
    assert set(rows["gn_twopass256"]) == {"gn_bwd_kernel[<256>]"}
    assert rows["gn_twopass1024"] == ["gn_bwd_kernel[<256>]"] * 5 + ["gn_bwd_kernel[<1024>]"] * 3


def test_the_conv1x1_table_reaches_what_it_claims():
    stages = [(s[1] + s[2]) // 16 for s in K.C1_CASES]
    assert min(stages) == 1 and 3 in stages and max(stages) == 16
    assert all(s[3] % 128 == 0 and s[4] * s[5] % 512 == 0 and s[4] * s[5] >= 1024 for s in K.C1_CASES)      # served by the <., 128> kernels
    assert any(s[3] == 256 for s in K.C1_CASES) and any(s[2] for s in K.C1_CASES) and any(s[6] for s in K.C1_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# fairness: the fp32 CPU evaluation of every case meets its bar against fp64

WORST = {}


@pytest.mark.parametrize("shape,kind", sorted({(K.CASES[k].shape, K.CASES[k].sub) for k in ATTN}), ids=lambda v: str(v).replace(" ", ""))
def test_the_bar_is_fair_to_fp32_attention(shape, kind):
    """PyTorch's fp32 autograd through the oracle meets the bar, and so does a forward whose scores are summed in fp32 in either
    unit system, natural (attention_kernel) or log 2 (the split and LDS-staged kernels), with everything else exact."""
    a64, g64 = K.attn_reference(shape, kind)
    a32, g32 = AB.autograd(*AB.inputs(K.attn_case(shape), kind), shape[1], torch.float32)
    ra, rg = AB.bar_ratio(a32, a64), AB.bar_ratio(g32, g64)
    units = {name: AB.bar_ratio(other_units_backward(shape, kind, b2, b2)[0], a64) for name, b2 in (("natural", False), ("log 2", True))}
    print(f"T{shape[2] * shape[3]}-{shape}-{kind}: fp32 autograd vs fp64, err / bar: a {ra:.4f}, dqkv {rg:.4f}; a from fp32 scores: "
          + ", ".join(f"{k} {v:.4f}" for k, v in units.items()))
    assert ra <= 1.0 and rg <= 1.0 and max(units.values()) <= 1.0, (ra, rg, units)


@pytest.mark.parametrize("shape", K.C1_CASES, ids=K.c1_key)
def test_the_bar_is_fair_to_fp32_conv1x1(shape):
    t = K.c1_inputs(shape)
    ref, got = K.c1_reference64(shape), K.c1_reference(t, torch.float32).double()
    r = float(((got - ref).abs() / (1e-5 + 1e-4 * ref.abs())).max())
    print(f"{K.c1_key(shape)}: fp32 conv vs fp64, err / bar {r:.4f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("shape", K.WINO_CASES, ids=K.wino_key)
def test_the_bar_is_fair_to_fp32_winograd_cases(shape):
    ref, got = K.wino_reference64(shape), K.wino_reference(K.wino_inputs(shape), torch.float32).double()
    r = float(((got - ref).abs() / (1e-5 + 1e-4 * ref.abs())).max())
    print(f"{K.wino_key(shape)}: fp32 conv vs fp64, err / bar {r:.4f}")
    assert r <= 1.0, r


@pytest.mark.parametrize("case", K.GN_CASES, ids=K.gn_key)
def test_the_bar_is_fair_to_fp32_groupnorm(case):
    ref, got = K.gn_reference64(case), K.gn_reference(case, K.gn_inputs(case), torch.float32)
    r = {k: AB.bar_ratio(got[k], ref[k]) for k in K.GN_OUT if ref[k] is not None}
    print(f"{K.gn_key(case)}: fp32 autograd vs fp64, err / bar: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


# ---------------------------------------------------------------------------------------------------------------------------------
# the mutant


def other_units_backward(shape, kind, fwd_base2, bwd_base2, fp32_scores=True):
    """fp64 (a, dqkv) of a forward / backward pair in which each side forms its scores in its own unit system (natural: q / 8;
    base 2: q log2(e) / 8) and everything after the scores is exact: a and delta = sum_c da a carry the forward's probabilities,
    dS = P (dP - delta) the backward's.  fp32_scores: the scaled query is rounded to fp32 and so is the 64-term sum of the score,
    as on the matrix pipe; without it only the scaled query is (one rounding, none at all in natural units: 1 / 8 is a power of 2)."""
    qkv, da = AB.inputs(K.attn_case(shape), kind)
    B, heads, H, W = shape
    q, k, v = (t.double() for t in qkv.reshape(B * heads, 64, 3, H * W).unbind(2))
    dA = da.double().reshape(B * heads, 64, H * W)
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)

    def probs(base2):
        scale = torch.tensor(0.125, dtype=torch.float32) * log2e if base2 else torch.tensor(0.125, dtype=torch.float32)
        qs = q.float() * scale
        s = torch.einsum("ncq,nck->nqk", qs, k.float()).double() if fp32_scores else torch.einsum("ncq,nck->nqk", qs.double(), k)
        return (s * math.log(2.0)).softmax(2) if base2 else s.softmax(2)
    Pf, Pb = probs(fwd_base2), probs(bwd_base2)
    a = torch.einsum("nqk,nck->ncq", Pf, v)
    delta = (dA * a).sum(1)                                    # [n, q]
    dP = torch.einsum("ncq,nck->nqk", dA, v)
    dS = Pb * (dP - delta[:, :, None])
    dq = torch.einsum("nqk,nck->ncq", dS, k) / 8
    dk = torch.einsum("nqk,ncq->nck", dS, q) / 8
    dv = torch.einsum("nqk,ncq->nck", Pb, dA)
    return a.reshape(B, heads * 64, H, W), torch.stack([dq, dk, dv], 2).reshape(qkv.shape)


SPLIT0_PAIRS = [K.CASES[k].shape for k in K.GROUPS["attn_split0"][1] if K.CASES[k].kind == "attn_pair"]


@pytest.mark.parametrize("shape", SPLIT0_PAIRS, ids=lambda s: f"T{s[2] * s[3]}")
def test_a_backward_in_the_other_units_is_outside_the_bar(shape):
    """What attn_split0's pairs are there to notice: the forward in natural units, the backward in units of log 2, each with its
    scores summed in fp32.  Scores of +-150 carry an fp32 rounding of 1e-5, i.e. a relative 1e-5 on a probability; where both
    sides form the SAME scores that error is in delta too and cancels in dS = P (dP - delta), where they do not it meets
    |dP - delta| of 100 and more.  One unit system on both sides is well inside the bar, so it is the mismatch that the bar
    sees.  (One fp32 rounding of the scaled query ALONE, with exact sums, is not enough: 0.04 to 0.16 of the bar on these cases.)"""
    _, g64 = K.attn_reference(shape, "x6")
    r = {"mixed": AB.bar_ratio(other_units_backward(shape, "x6", False, True)[1], g64),
         "mixed, q rounded only": AB.bar_ratio(other_units_backward(shape, "x6", False, True, fp32_scores=False)[1], g64)}
    for b2 in (False, True):
        r["base2" if b2 else "natural"] = AB.bar_ratio(other_units_backward(shape, "x6", b2, b2)[1], g64)
    print(f"T{shape[2] * shape[3]}: dqkv err / bar vs fp64: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert r["natural"] <= 1.0 and r["base2"] <= 1.0, r
    if shape[2] * shape[3] == 129:      # the one T of the table at which this model stays inside the bar (0.91 at 8 heads, 0.84 at 16)
        assert r["mixed"] > 2 * max(r["natural"], r["base2"]), r
    else:
        assert r["mixed"] > 1.0, r
