"""cdx_hand_term on the host build (libcdx_host.so's cdxh_hand_term, the same cdx_hand.h rows the kernel runs): the
term against cdx_hand_cost followed by cdx_hand_pullback and against numpy's old + (weight · x), bit for bit; rows,
guard rows and refusals (tests/_hand_term.py).  No GPU."""
import pytest

from tests import _chains, _hand as H, _hand_term as T


@pytest.mark.parametrize("case,S,pairs", T.FAMILIES, ids=T.IDS)
def test_term_is_the_pair_and_the_output_rule(case, S, pairs):
    T.check_values(T.HostBackend, T.fam(case, S, pairs))


@pytest.mark.parametrize("case,S,pairs", T.FAMILIES[:3], ids=T.IDS[:3])
def test_rows_stay_in_their_row(case, S, pairs):
    T.check_rows(T.HostBackend, T.fam(case, S, pairs))


def test_refusals_leave_the_outputs_untouched():
    T.check_refusals(T.HostBackend, T.fam("hand8", 63, "full"), H.family("tree8", 65, "one")["hs"],
                     _chains.raw_descriptor(_chains.line(17), ["b17"]))


def test_hand_term_value_type():
    """HandTerm: the fields of the issue, exported from the package, refusing non-finite numbers and a wrong model."""
    import compliancedex_amd as cdx
    hs = H.family("hand8", 63, "full")["hs"]
    t = cdx.HandTerm(hs)
    assert (t.hand, t.weight, t.m_obj, t.m_self, t.m_floor, t.w_obj, t.w_self, t.w_floor, t.floor_z, t.obj) == \
        (hs, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, None, None)
    t = cdx.HandTerm(hs, weight=0.5, m_obj=0.01, floor_z=-0.1, w_self=3.0)
    p = t.params()
    assert (p.m_obj, p.w_self, p.floor_on, p.floor_z) == (0.01, 3.0, 1, -0.1) and t.params().floor_on == 1
    assert cdx.HandTerm(hs).params().floor_on == 0
    assert t.key(None) != cdx.HandTerm(hs, weight=0.25, m_obj=0.01, floor_z=-0.1, w_self=3.0).key(None)
    with pytest.raises(ValueError):
        cdx.HandTerm(hs, weight=float("nan"))
    with pytest.raises(TypeError):
        cdx.HandTerm("allegro")
    with pytest.raises(ValueError):
        t.check(hs.desc.n_dofs + 1, "cuda")
