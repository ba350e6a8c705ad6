"""--split-device gpu of the `bert` and `bart` sub-commands: the same output
files, byte for byte, as --split-device host over about 200 KB of synthetic
records in three files (BERT: several pipeline chunks, binned), the timing
keys of the route, and what it refuses: the codebert sub-command, a splitter
other than the rule-based one, a record that is not UTF-8 (the
UnicodeDecodeError of the host route)."""
import os

import pytest

import split_model as M
from lddl_amd import preprocess

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def encode_in_threads(monkeypatch):
  """(the parquet encodes on threads: forking encoder processes from a test process that holds many GPU
  contexts takes seconds, and the files are the same)"""
  monkeypatch.setenv('LDDL_ENCODE_PROCS', '0')
  monkeypatch.setenv('LDDL_CPU_SHARE', '2')  # (bart: two gathering workers are forked, not one per partition)


@pytest.fixture(scope='module')
def wiki_dir(gpu, tmp_path_factory):
  root = tmp_path_factory.mktemp('split_cli')
  src = root / 'wiki' / 'en'
  src.mkdir(parents=True)
  recs = M.wiki(200_000, seed=21)
  for k in range(3):
    with open(str(src / ('wiki_%d.txt' % k)), 'w', encoding='utf-8') as f:
      for r in recs[k::3]:
        f.write(r + '\n')
  return root


def tree(d):
  return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def test_bert_same_files(wiki_dir):
  out, t = {}, {}
  for dev in ('host', 'gpu'):
    sink = wiki_dir / ('bert_' + dev)
    args = preprocess.attach_args().parse_args(
        ['--wikipedia', str(wiki_dir / 'wiki'), '--sink', str(sink), '--target-seq-length', '128', '--bin-size', '32',
         '--num-blocks', '8', '--chunk-mb', '0.02', '--sentence-splitter', 'rules', '--seed', '5',
         '--split-workers', '0', '--split-device', dev])
    files, t[dev] = preprocess.main(args)
    out[dev] = tree(str(sink))
    assert len(files) == len(out[dev]) > 0
  assert t['gpu']['chunks'] >= 3 and t['gpu']['chunks'] == t['host']['chunks']
  assert sorted(out['gpu']) == sorted(out['host'])
  for f in out['host']:
    assert out['gpu'][f] == out['host'][f], f
  assert t['gpu']['sentence_splitter'] == 'rules-gpu' and t['host']['sentence_splitter'] == 'rules'
  assert t['gpu']['gpu_split_s'] > 0 and 'gpu_split_s' not in t['host']
  assert t['gpu']['pairs'] == t['host']['pairs'] > 0


def test_bart_same_files(wiki_dir):
  out, t = {}, {}
  for dev in ('host', 'gpu'):
    sink = wiki_dir / ('bart_' + dev)
    args = preprocess.bart_parser().parse_args(
        ['--wikipedia', str(wiki_dir / 'wiki'), '--sink', str(sink), '--target-seq-length', '128', '--num-blocks', '6',
         '--sentence-splitter', 'rules', '--split-device', dev])
    files, t[dev] = preprocess.bart_main(args)
    out[dev] = tree(str(sink))
    assert len(files) == len(out[dev]) > 0
  assert sorted(out['gpu']) == sorted(out['host'])
  for f in out['host']:
    assert out['gpu'][f] == out['host'][f], f
  assert t['gpu']['sentence_splitter'] == 'rules-gpu' and t['gpu']['gpu_split_s'] > 0
  assert t['gpu']['chunks_out'] == t['host']['chunks_out'] > 0


def test_refused_combinations(wiki_dir, monkeypatch):
  common = ['--sink', str(wiki_dir / 'never'), '--split-device', 'gpu']
  with pytest.raises(ValueError, match='codebert'):
    preprocess.main(preprocess.attach_args(codebert=True).parse_args(common + ['--code', str(wiki_dir / 'wiki')]),
                    codebert=True)
  # a resolved splitter other than the rules: named, with the flag that selects them
  monkeypatch.setattr(preprocess, 'sentence_splitter', lambda kind='auto': (str.split, 'punkt'))
  for kind in ('punkt', 'auto'):
    with pytest.raises(ValueError, match='--sentence-splitter rules'):
      preprocess.main(preprocess.attach_args().parse_args(
          common + ['--wikipedia', str(wiki_dir / 'wiki'), '--sentence-splitter', kind]))
    with pytest.raises(ValueError, match='--sentence-splitter rules'):
      preprocess.bart_main(preprocess.bart_parser().parse_args(
          common + ['--wikipedia', str(wiki_dir / 'wiki'), '--sentence-splitter', kind]))
  assert not os.path.exists(str(wiki_dir / 'never'))


@pytest.mark.parametrize('dev', ['host', 'gpu'])
def test_invalid_utf8_raises_on_both_routes(gpu, tmp_path, dev):
  src = tmp_path / 'wiki' / 'en'
  src.mkdir(parents=True)
  (src / 'a.txt').write_bytes(b'doc1 A fine record. Two sentences.\ndoc2 a bad \xff byte. Here.\ndoc3 Fine again. Yes.\n')
  argv = ['--wikipedia', str(tmp_path / 'wiki'), '--sink', str(tmp_path / 'o'), '--sentence-splitter', 'rules',
          '--split-device', dev]
  with pytest.raises(UnicodeDecodeError):
    preprocess.main(preprocess.attach_args().parse_args(argv + ['--split-workers', '0', '--sample-ratio', '1.0']))
  with pytest.raises(UnicodeDecodeError):
    preprocess.bart_main(preprocess.bart_parser().parse_args(argv))
