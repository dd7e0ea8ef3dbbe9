"""The binding's stride rule for feature tensors (_feature_strides, under FeatureNorm and FrameStack) on the CPU, against the
library's own (alacfv::layout_of behind the host build of the normalisation pass, tests/host_sim/featnorm_sim.cpp).

Views of the logical shapes [R, F, B] with R in {1, 3}, F in {1, 4}, B in {1, 5}, as torch CPU tensors [R, F, B] (layout
"frames") and [R, B, F] ("bins"): the tensor itself, [..., :-1], [:, :-1], [:, ::2], [..., ::2] and the transpose of the inner
axes read as the other layout, each cut out of a base that is larger by what the slice drops, so that every view has the full
shape. Slices and transposes only: over as_strided and overlapping frames the binding and the library knowingly differ.

* the rule returns None exactly where the host build refuses torch's own strides with -2, but for [..., ::2] where F or B is 1:
  there the rule replaces the stride of the one-element axis by 1 and takes the view, while the library, given torch's own
  strides, finds no inner stride of 1 and refuses. That was so before the rule moved out of FeatureNorm and is not this test's
  to settle: it is asserted as it stands, so that it does not change unnoticed;
* where the rule returns strides, those cases included, the host build on those strides returns 0 and gives the bits of
  featnorm_ref.reference (stat mean)."""
import numpy as np
import pytest

from tests import featnorm_ref as fr


@pytest.fixture(scope="module")
def sim():
    return fr.build_featnorm_sim()


def views_of(torch, x, layout):
    """x [R, F, B] numpy -> {name: a torch view that holds x as [R, F, B] (frames) or [R, B, F] (bins)}"""
    t = torch.from_numpy(x if layout == "frames" else np.ascontiguousarray(x.transpose(0, 2, 1)))
    R, a, b = t.shape

    def inside(shape, cut):
        base = torch.full(shape, float("nan"))
        base[cut] = t
        return base[cut]

    return {
        "itself": t.clone(),
        "[..., :-1]": inside((R, a, b + 1), (Ellipsis, slice(None, -1))),
        "[:, :-1]": inside((R, a + 1, b), (slice(None), slice(None, -1))),
        "[:, ::2]": inside((R, 2 * a, b), (slice(None), slice(None, None, 2))),
        "[..., ::2]": inside((R, a, 2 * b), (Ellipsis, slice(None, None, 2))),
        "transpose": t.transpose(1, 2).contiguous().transpose(1, 2),
    }


@pytest.mark.parametrize("layout", ["frames", "bins"])
def test_stride_rule_against_the_host_build(pkg, sim, layout):
    import torch
    rng = np.random.default_rng(5)
    refused = taken = 0
    for R in (1, 3):
        for F in (1, 4):
            for B in (1, 5):
                x = fr.features(rng, R, F, B)
                want = fr.reference(x, None, "mean")[0]
                for name, v in views_of(torch, x, layout).items():
                    case = "%s of %s, layout %s" % (name, (R, F, B), layout)
                    assert tuple(v.shape) == ((R, F, B) if layout == "frames" else (R, B, F)), case
                    rs, s1, s2 = (int(s) for s in v.stride())
                    own = (rs, s1, s2) if layout == "frames" else (rs, s2, s1)
                    obuf, oview, ost = fr.lay_out(np.zeros_like(x), layout)
                    rc = fr.host_run(sim, B, v.data_ptr(), own, R, F, None, oview.ctypes.data, ost, stat="mean")
                    st = pkg._feature_strides(v, layout)
                    said = "%s: the rule gives %r, the host build %d on %r" % (case, st, rc, own)
                    if name == "[..., ::2]" and 1 in (F, B):  # the known difference, held as it is
                        assert st is not None and rc == -2, said
                    else:
                        assert rc in (0, -2) and (st is None) == (rc == -2), said
                    if st is None:
                        refused += 1
                        continue
                    taken += 1
                    obuf, oview, ost = fr.lay_out(np.zeros_like(x), layout)
                    assert fr.host_run(sim, B, v.data_ptr(), st, R, F, None, oview.ctypes.data, ost, stat="mean") == 0, case
                    assert fr.same_bits(oview, want), case
    assert refused and taken
