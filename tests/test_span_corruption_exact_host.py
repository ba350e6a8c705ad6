"""span_corruption_lengths (lddl_corrupt_exact_lengths): the closed-form lengths of exact-count span corruption against
tests/segment_model.py's counts; host only."""
import pytest

import segment_model as sg
from lddl_amd import loader

LAWS = [(0.15, 3.0), (0.5, 1.0), (0.3, 1000.0)]


@pytest.mark.parametrize('law', LAWS)
@pytest.mark.parametrize('count', [99, 5, 4096])
def test_lengths_against_the_model(law, count):
  for n in range(2, 2049):
    assert loader.span_corruption_lengths(n, *law, num_sentinels=count) == sg.lengths(n, *law, count), n


def test_rint_ties_round_to_even():
  assert loader.span_corruption_lengths(12, 0.25, 1.0)[2:] == (2, 2)       # c = 10: 2.5 -> 2
  assert loader.span_corruption_lengths(16, 0.25, 1.0)[2:] == (4, 4)       # c = 14: 3.5 -> 4
  assert loader.span_corruption_lengths(12, 0.5, 2.0) == (12 - 5 + 2, 5 + 2 + 1, 5, 2)  # N / mean = 2.5 -> 2
  assert loader.span_corruption_lengths(3, 0.9, 1.0) == (3, 1, 0, 0)       # c < 2: the row passes unchanged
  assert loader.span_corruption_lengths(4, 0.9, 1.0) == (4, 3, 1, 1)       # N <= c - 1


@pytest.mark.parametrize('bad', [dict(n=1), dict(noise_density=0.0), dict(noise_density=1.0), dict(mean_span=0.5),
                                 dict(mean_span=float('inf')), dict(num_sentinels=0), dict(n=2049)])
def test_refusals(bad):
  with pytest.raises(RuntimeError):
    loader.span_corruption_lengths(**{'n': 100, **bad})
