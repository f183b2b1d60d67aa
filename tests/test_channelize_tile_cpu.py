"""The tile rule the front end's GPU tests share (channelize_tile.py), on the CPU."""
import channelize_tile as CT


def test_a_real_capture_always_gets_four_slots_per_lane():
    """k_channelize.hip instantiates the ratio form for a real capture at NP = 4 only and proves with a static_assert that
    rechannelize_shape never asks for another: the same walk over every admitted ratio, through the tests' restatement of the rule"""
    ratios = CT.admitted_ratios()
    assert len(ratios) == 2370
    assert {CT.tile_shape(p, q, 4)[1] for p, q in ratios} == {4}
    assert {CT.tile_shape(d, 1, 4) for d in range(2, 33)} == {(256, 4)}


def test_an_analytic_capture_uses_every_slot_count():
    """(the ratios the GPU tests run at NP = 4, 2, 3 and 1, and how many admitted ratios select NP = 3 and NP = 1)"""
    assert [CT.tile_shape(p, q, 8) for p, q in ((5, 2), (125, 4), (49, 2), (472, 15))] == [(256, 4), (128, 2), (192, 3), (60, 1)]
    per_lane = [CT.tile_shape(p, q, 8)[1] for p, q in CT.admitted_ratios()]
    assert per_lane.count(3) == 329
    assert [pq for pq in CT.admitted_ratios() if CT.tile_shape(*pq, 8)[1] == 1] == [(472, 15), (473, 15), (476, 15), (478, 15), (479, 15)]
    assert [CT.tile_shape(d, 1, 8) for d in (2, 16, 17, 32)] == [(256, 4), (256, 4), (128, 2), (128, 2)]
