"""The default full stop of collate_denoise (loader.default_full_stop): a lookup in the vocabulary, no ctx."""
import pytest

from lddl_amd import _lib, loader
from lddl_amd.tokenizer import vocab_entries


def test_default_full_stop():
  assert vocab_entries(_lib.VOCAB_BERT)[loader.default_full_stop(_lib.VOCAB_BERT)] == '.'
  assert loader.default_full_stop({'a': 5, '.': 9}) == 9
  with pytest.raises(ValueError, match='full_stop'):
    loader.default_full_stop({'a': 5, '##.': 9})
