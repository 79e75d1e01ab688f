"""The zpack entropy stage, measured ON THE MODEL (writes profiles/chunk_zentropy_model.txt).  CPU only.

The stored bytes are a property of the model, which the kernels reproduce byte for byte, so the ratio is settled here.  The corpus
is that of profiles/chunk_zpack_l2_model.txt (tools/zpack_model_ratio.py's: regular files under /usr/lib, largest first, the
first `per_file` bytes of each, cut in 8 KiB pieces).  Every piece is stored at level 1 and at level 2, each without the stage
and with it (zentropy_cases.compress_chunk_h: form H kept where it is smaller by more than a sixteenth); the stage is sized with
16, 32 and 64 streams and with an unlimited Huffman code in place of the 11-bit one.  Every form H of the 32-stream rows is built
and decoded again with the model's decoder.  THE CONDITION the design stands on is asserted: level 1 with the stage stores fewer
bytes than level 2 without it.
zentropy_model_ratio.py [out = profiles/chunk_zentropy_model.txt] [bytes = 3e6] [per_file = 262144]"""
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import zentropy_cases as ze
    from zpack_model_ratio import corpus
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zentropy_model.txt")
    limit = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000
    per_file = int(float(sys.argv[3])) if len(sys.argv) > 3 else 262144
    pieces, names, total = corpus(limit, per_file)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("zpack entropy stage, the model's ratio (tools/zentropy_model_ratio.py %d %d): %d bytes in %d pieces of 8192, the first %d bytes of each of"
        % (limit, per_file, total, len(pieces), per_file))
    for path, n in names:
        say("        %9d  %s" % (n, path))
    yard = sum(len(zlib.compress(p, 1)) for p in pieces)
    t0 = time.perf_counter()
    under = dict((lv, [ze.under_form(p, lv) for p in pieces]) for lv in (1, 2))
    plain = dict((lv, sum(len(u) for u in under[lv])) for lv in (1, 2))
    one = plain[1]
    say("(the two parses: %.0f s)" % (time.perf_counter() - t0))
    say("%-52s %10s %9s %9s %9s %8s" % ("form", "stored", "/ input", "/ level 1", "/ zlib -1", "H rows"))

    def row(name, stored, n_h=None):
        say("%-52s %10d %9.4f %9.4f %9.4f %8s" % (name, stored, stored / total, stored / one, stored / yard, "" if n_h is None else n_h))

    def staged(forms, streams, bits):
        """the stored bytes with the stage on, and how many pieces took form H"""
        stored = n_h = 0
        for u in forms:
            h = ze.huff_size(u, streams, bits)
            keep = h < len(u) - (len(u) >> 4)
            stored += h if keep else len(u)
            n_h += keep
        return stored, n_h

    row("zlib.compress(piece, 1)", yard)
    result = {}
    for lv in (1, 2):
        row("level %d" % lv, plain[lv])
        for streams in (16, 32, 64):
            result[lv, streams] = staged(under[lv], streams, ze.MAX_BITS)
            row("level %d + stage, %d streams, 11-bit code" % (lv, streams), *result[lv, streams])
        row("level %d + stage, 32 streams, unlimited code" % lv, *staged(under[lv], 32, None))
    row("the stage over the plain bytes alone, 32 streams", *staged(pieces, 32, ze.MAX_BITS))
    t0 = time.perf_counter()
    for lv in (1, 2):                                              # the forms themselves: built, measured, decoded again
        stored = 0
        for p in pieces:
            s = ze.compress_chunk_h(p, lv)
            assert ze.expand_chunk(s, len(p)) == p
            stored += len(s)
        assert stored == result[lv, 32][0], (lv, stored, result[lv, 32])
    say("(every form of the 32-stream rows built and decoded again by the model's decoder: %.0f s)" % (time.perf_counter() - t0))
    say("the condition: level 1 + stage (%d) < level 2 alone (%d): %s" % (result[1, 32][0], plain[2], result[1, 32][0] < plain[2]))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert result[1, 32][0] < plain[2], "the design's condition does not hold"


if __name__ == "__main__":
    main()
