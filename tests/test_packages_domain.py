"""The package bank's domain cases without a GPU: the carry grid and the composed cases of tests/test_gpu_packages_domain.py checking
themselves, and the kernel's placement of a run of bits in the carried 256 (word_of) modelled on the grid's data -- as it is, where it
gives the definition's bits, and without its branch for a run that begins inside a word, where it does not."""
import pytest

import packages_cases as kc
import packages_domain_cases as dc


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_case_table_checks_itself(name):
    assert dc.case(name).name == name and name not in kc.CASE_NAMES
    dc.check_case(name)


def test_the_grid_reaches_every_branch_of_the_placement():
    """d = 32 w - p over the eight words: d >= 0, -32 < d < 0 and d <= -32 each occur, at p on, in front of and behind a multiple of
    32, and p + n lies on either side of 256."""
    seen = set()
    for p, n in dc.grid_pairs():
        for w in range(8):
            d = 32 * w - p
            seen.add("ge" if d >= 0 else "inside" if d > -32 else "below")
    assert seen == {"ge", "inside", "below"}
    assert {p % 32 for p in dc.GRID_P} >= {0, 1, 31} and {n for n in dc.GRID_N} >= {1, 32, 33, 64}
    sums = {p + n for p, n in dc.grid_pairs()}
    assert {255, 256, 257} <= sums and max(sums) == 320


@pytest.mark.parametrize("m", ["pwm", "ppm"])
def test_the_placement_model_gives_the_grids_bits_and_not_without_its_branch(m):
    per_call, _ = dc.expected("carry_grid_" + m)
    differ = set()
    for s, (p, n) in enumerate(dc.grid_pairs()):
        k, bits = per_call[1][1][s][0], dc.grid_bits(p, n)
        want = (kc.bits_of(k) + [0] * 256)[:256]
        assert dc.appended(bits, min(p, 256)) == want, (p, n)
        if dc.appended(bits, min(p, 256), negative=False) != want:
            differ.add(p)
    # a run that begins inside a word loses its first bits without the branch: every such p shows it at some n
    assert differ == {p for p in dc.GRID_P if p % 32 and p < 256}, sorted(differ)


@pytest.mark.parametrize("m", ["pwm", "ppm"])
@pytest.mark.parametrize("n_streams", dc.COMPOSED_STREAMS)
def test_composed_cases_check_themselves(fmd, n_streams, m):
    dc.check_composed(n_streams, m)
