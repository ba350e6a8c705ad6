"""The default sentinels of collate_span_corruption (loader.default_sentinels): a lookup in the vocabulary file, no ctx."""
import pytest

from lddl_amd import _lib, loader


def test_default_sentinels():
  assert loader.default_sentinels(_lib.VOCAB_BERT) == (1, 99)  # [unused0] .. [unused98]; [unused99] follows [MASK]
  assert loader.default_sentinels({'[unused0]': 7, '[unused1]': 8, '[unused2]': 10}) == (7, 2)
  with pytest.raises(ValueError, match='sentinels'):
    loader.default_sentinels(_lib.VOCAB_CODEBERT)
