"""The host-side restatements of tests/wide_linear_cases.py on the numbers their sources state (no GPU): the row deals of
launch_linear_big_impl / launch_linear_short on a 256-CU chip, the width up to which a net stays on the LDS-resident
kernels, and the layout of a packed copy."""
import wide_linear_cases as W


def test_big_deal_on_256_cus_at_10_panels():
    """latent 1280: 10 panels, 52 workgroups per panel in the first round"""
    want = {103: (1, 51, 1), 104: (2, 0, 1), 130: (2, 26, 1), 156: (3, 0, 1), 204: (3, 48, 1), 205: (1, 102, 2)}
    for tiles, (base, rem, rounds) in want.items():
        for n in (16 * tiles, 16 * tiles - 15):
            d = W.big_deal(n, 1280, 256)
            assert (d["wg_base"], d["wg_rem"], d["rounds"], d["panels"]) == (base, rem, rounds, 10), (tiles, d)
    assert W.big_deal(1640, 1280, 256)["wpp"] == 52
    assert W.big_deal(16 * 102, 1280, 256) is None            # fewer than two row-tile units per CU slot
    assert W.big_deal(3257, 1280, 256)["sizes"] == {3, 4} and W.big_deal(3280, 1280, 256)["sizes"] == {1, 2}
    # the data driver's batch (gnf_linear_big.hip): 170 row tiles, 16 panels -> 42 x 3 + 22 x 2
    d = W.big_deal(2718, 2048, 256)
    assert (d["wpp"], d["wg_base"], d["wg_rem"]) == (64, 2, 42)


def test_short_deal_instances_and_rounds():
    inst = {4: "7x4", 100: "7x4", 112: "7x4", 128: "8x4", 132: "11x2", 144: "11x2", 164: "11x2", 176: "11x2", 180: "13x2", 208: "13x2"}
    for i, name in inst.items():
        assert W.short_deal(1664, i, 1280, 256)["instance"] == name, i
    for refused in (7, 150, 212, 256):
        assert W.short_deal(1664, refused, 1280, 256) is None
    assert W.short_deal(1664, 100, 1030, 256) is None          # O & 3
    d = W.short_deal(1640, 144, 1280, 256)
    assert (d["panels"], d["wg_base"], d["wg_rem"], d["rounds"]) == (20, 3, 25, 1)
    d = W.short_deal(6560, 144, 1280, 256)
    assert (d["wg_base"], d["wg_rem"], d["rounds"]) == (7, 46, 2)


def test_lds_resident_kernels_hold_hidden_widths_up_to_about_1100():
    """gnf_fused.hip: "(*,1) ... keeps layers up to 1024 wide on the fused path" - a net 100 -> L -> L -> 100"""
    for latent in (512, 528, 1024, 1030, 1040):
        assert W.fused_fwd_fits([100, latent, latent, 100]), latent
    for latent in (1280, 1536, 2048):
        assert not W.fused_fwd_fits([100, latent, latent, 100]) and not W.fused_bwd_fits([100, latent, latent, 100])
    assert W.fused_bwd_fits([32, 256, 256, 256, 256, 32]) and not W.fused_bwd_fits([150, 512, 512, 150])
    assert not W.fused_fwd_fits([1200, 512, 512, 1200])        # another width of the net is what counts
    assert W.wide_only([12, 1280, 1280, 12]) and not W.wide_only([100, 1040, 1040, 100])


def test_packed_regions_tile_a_nets_copy():
    dims = [100, 1040, 1030, 7]
    spans = sorted(W.packed_region(dims, kind, j) for kind in ("w", "b", "wt") for j in range(3))
    end = 0
    for off, ln in spans:
        assert off == end
        end = off + ln
    assert end == W.packed_floats(dims)
    assert W.packed_region(dims, "b", 0) == (112 * 1040 + 1040 * 1040 + 1040 * 16, 1040)
    assert [W.net_index(k, h) for k in ("s", "t") for h in (0, 1)] == [0, 1, 2, 3]
    assert W.fused_last([100, 1280, 1280, 100], 2) and not W.fused_last([150, 1280, 1280, 150], 2)
    assert not W.fused_last([100, 1280, 100], 1)
