"""Region plan of the attention-carried weight prefetch (CPU)."""

from llm_np_cp_amd.models.attn_prefetch import (consumer_stride,
                                                default_budget,
                                                plan_attn_prefetch)

H, I = 2048, 8192
WO, WGU = H * H * 2, 2 * I * H * 2      # Llama-3.2-1B, bf16
ROW = H * 2


def aligned(regions):
    return all(off % 16 == 0 and n % 16 == 0 and n > 0
               for _, off, n in regions)


def test_budget_zero_gives_nothing():
    assert plan_attn_prefetch(WO, WGU, I, H, 0) == []
    assert plan_attn_prefetch(WO, WGU, I, H, -5) == []


def test_budget_below_wo_gives_a_prefix_of_wo():
    assert plan_attn_prefetch(WO, WGU, I, H, 1 << 20) == [("wo", 0, 1 << 20)]
    # rounded down to whole 16 B
    assert plan_attn_prefetch(WO, WGU, I, H, 1000) == [("wo", 0, 992)]
    assert plan_attn_prefetch(WO, WGU, I, H, WO) == [("wo", 0, WO)]


def test_budget_between_gives_wo_and_equal_gate_up_heads():
    r = plan_attn_prefetch(WO, WGU, I, H, WO + (32 << 20))
    assert r[0] == ("wo", 0, WO)
    (n1, gate_off, gate_n), (n2, up_off, up_n) = r[1:]
    assert n1 == n2 == "wgu"
    assert gate_off == 0 and up_off == I * ROW
    assert gate_n == up_n == 16 << 20
    assert gate_n % ROW == 0            # whole rows
    assert aligned(r)
    # a remainder smaller than one gate row + one up row buys nothing
    assert plan_attn_prefetch(WO, WGU, I, H, WO + 2 * ROW - 1) == r[:1]
    assert plan_attn_prefetch(WO, WGU, I, H, WO + 2 * ROW)[1:] == [
        ("wgu", 0, ROW), ("wgu", I * ROW, ROW)]


def test_budget_above_everything_gives_whole_tensors_only():
    for budget in (WO + WGU, WO + WGU + 12345, 1 << 40):
        r = plan_attn_prefetch(WO, WGU, I, H, budget)
        assert r == [("wo", 0, WO), ("wgu", 0, WGU // 2),
                     ("wgu", WGU // 2, WGU // 2)]
        size = {"wo": WO, "wgu": WGU}
        assert all(off + n <= size[name] for name, off, n in r)


def test_odd_sizes_stay_aligned_and_inside():
    # K = 1000 fp8 bytes per row is not a multiple of 16: up rows would
    # start unaligned, so only wo is planned
    assert plan_attn_prefetch(4000, 2 * 6 * 1000, 6, 1000, 1 << 20) == [
        ("wo", 0, 4000 & ~15)]
    r = plan_attn_prefetch(4096 * 48, 2 * 100 * 48, 100, 48, 4096 * 48 + 1000)
    assert aligned(r) and r[1:] == [("wgu", 0, 480), ("wgu", 4800, 480)]


def test_moe_layers_get_none():
    assert plan_attn_prefetch(WO, WGU, I, H, WO + WGU, moe=True) == []


def test_fp8_and_fp4_use_the_quantized_byte_sizes():
    r8 = plan_attn_prefetch(WO // 2, WGU // 2, I, H, WO // 2 + (8 << 20))
    assert r8 == [("wo", 0, WO // 2), ("wgu", 0, 4 << 20),
                  ("wgu", I * H, 4 << 20)]
    r4 = plan_attn_prefetch(WO // 4, WGU // 4, I, H, 1 << 40)
    assert r4 == [("wo", 0, WO // 4), ("wgu", 0, WGU // 8),
                  ("wgu", I * H // 2, WGU // 8)]


def test_consumer_stride_and_default_budget():
    assert consumer_stride(WO, H, 4) == 4 * ROW
    assert consumer_stride(WO // 2, H, 4) == 2 * ROW
    assert consumer_stride(1000, 3, 4) == 0          # rows not whole
    assert consumer_stride(6 * 100, 100, 1) == 0     # unaligned stride
    # default: wo whole while it fits the attention window, else nothing
    assert default_budget(WO, WGU) == WO
    assert default_budget(WO // 2, WGU // 2) == WO // 2
    assert default_budget(4 * WO, 4 * WGU) == 0
    assert plan_attn_prefetch(WO, WGU, I, H, default_budget(WO, WGU)) == [
        ("wo", 0, WO)]
