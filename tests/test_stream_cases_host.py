"""The inputs of the side-stream cases (tests/stream_cases.py), without a GPU:
for every case, A and B of every staged array are built with numpy and held to
the rule that keeps a failing case a wrong answer and never a fault -- equal
shapes, no offset array staged, B lengths <= A lengths, payload inside its
range, text with every byte's role and every space in place, A != B."""
import numpy as np
import pytest

import stream_cases as SC


@pytest.mark.parametrize('case', SC.CASES, ids=[c.id for c in SC.CASES])
def test_staged_pairs_keep_the_rule(case):
  rng = np.random.default_rng(abs(hash(case.id)) % (1 << 32))
  meta = SC.meta_for(case)
  assert case.host or case.staged, 'a device case stages something'
  for name, role in case.staged:
    a = SC.host_stand_in(name, meta['vocab'], rng)
    b = SC.make_b(role, a, meta)
    SC.check_pair(name, role, a, b, meta)
    # a half-done copy: any element-wise mixture keeps the rule against A as well
    mix = np.where(rng.random(a.shape) < 0.5, a, b)
    SC.ROLES[role][1](a, mix, meta)


def test_case_ids_are_unique_and_roles_known():
  assert len({c.id for c in SC.CASES}) == len(SC.CASES)
  assert all(role in SC.ROLES for c in SC.CASES for _, role in c.staged)


@pytest.mark.parametrize('role,bad', [
    ('text', lambda a: np.where(a == 32, 97, a).astype(a.dtype)),       # a space became a letter
    ('ids', lambda a: a + 40000),                                       # outside the vocabulary
    ('lengths', lambda a: a + 1),                                       # B > A
    ('flags', lambda a: a ^ 2),                                         # the layout bit
    ('num_tokens', lambda a: a * 0),                                    # length 0: below the range
])
def test_the_rule_refuses_what_it_should(role, bad):
  rng = np.random.default_rng(7)
  meta = {'vocab': 30522, 'special': (0, 100, 101, 102, 103), 'range': (1, 129)}
  name = {'text': 'text', 'ids': 'ids', 'lengths': 'ntok', 'flags': 'flags', 'num_tokens': 'num_tokens'}[role]
  a = SC.host_stand_in(name, 30522, rng)
  with pytest.raises(AssertionError):
    SC.check_pair(name, role, a, bad(a), meta)


def test_offsets_are_never_staged():
  a = np.arange(10, dtype=np.int64)
  with pytest.raises(AssertionError):
    SC.check_pair('tok_off', 'values', a, a + 1, {})
