"""A plain model of the split tokenizer's scan windows, written from the rules
(DESIGN.md section 3), shared by tests/test_fb_cap_host.py and
tests/test_tokenize_dense_gpu.py:

  - tile t holds the sentences whose first byte lies in [1024 t, 1024 (t+1))
    relative to sent_off[0]; a call has nbytes // 1024 + 1 tiles;
  - a segment is seg tiles (at most all of them), a super-tile 16 tiles counted
    from its segment's first tile;
  - inside a super-tile's sentences [cs, ce) a window starts at sentence cs,
    a = sent_off[cs], aoff = (base_align + a) & 15, and takes further
    sentences i = 1..31 while cs + i <= ce and
    sent_off[cs + i] <= a - aoff + 2048; it holds max(count, 1) sentences.

Every window may be listed for the serial path, so the list's capacity has to
cover a segment's windows."""
from bisect import bisect_left, bisect_right

TILE = 1024
SUPER = 16
CAP = 2048
NS_MAX = 31


def tile_count(nbytes):
  return nbytes // TILE + 1


def old_cap(seg):
  """ranges the list held before it was sized by the sentence count too"""
  return 2 * seg + 64


def windows(sent_off, seg, base_align=0):
  """[(cs, ns), ...] per segment: the windows of a call over sent_off
  (n_sent + 1 offsets) with segments of min(seg, tiles) tiles"""
  off = [int(x) for x in sent_off]
  n_sent = len(off) - 1
  base = off[0]
  nt = tile_count(off[-1] - base)
  seg = min(seg, nt)
  starts = off[:n_sent]

  def tile_sent(t):  # first sentence starting at or after tile t
    return bisect_left(starts, base + t * TILE)
  out = []
  for t0 in range(0, nt, seg):
    t1 = min(nt, t0 + seg)
    ws = []
    for ta in range(t0, t1, SUPER):
      cs, ce = tile_sent(ta), tile_sent(min(t1, ta + SUPER))
      while cs < ce:
        a = off[cs]
        aoff = (base_align + a) & 15
        # offsets are sorted: the sentences that fit are a prefix
        fit = bisect_right(off, a - aoff + CAP, cs + 1, min(ce, cs + NS_MAX) + 1) - (cs + 1)
        ns = max(fit, 1)
        ws.append((cs, ns))
        cs += ns
    out.append(ws)
  return out


def too_long(sent_off, cs, ns, base_align=0):
  """the window's bytes from its aligned start pass 2048: one sentence too
  long for a window, which the scan hands to the serial path"""
  a = int(sent_off[cs])
  return int(sent_off[cs + ns]) - a + ((base_align + a) & 15) > CAP
