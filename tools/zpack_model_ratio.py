"""Zpack level 2's parse, measured ON THE MODEL (writes profiles/chunk_zpack_l2_model.txt).  CPU only.

The stored bytes are a property of the parse, and the kernel reproduces the model byte for byte, so the ratio is settled here.
The corpus is that of README's ratio figure: regular files under /usr/lib of the box, largest first, the first `per_file` bytes of
each until `bytes` are read, cut in 8 KiB pieces.  Every piece is coded by level 1's model (zpack_cases.compress_chunk), by level
2's model with each element (a) to (d) alone, with each element left out, and with all four (zpack2_cases.compress_chunk2), and
by zlib.compress(piece, 1).  Every level-2 block is decoded again with the independent decoder.
zpack_model_ratio.py [out = profiles/chunk_zpack_l2_model.txt] [bytes = 3e6] [per_file = 262144]"""
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PIECE = 8192
ELEMENTS = ["two_tables", "choose", "backward", "dense"]
LETTER = dict(zip(ELEMENTS, "acbd"))       # (b) per-lane lengths and (c) the choice are one switch: the choice is what uses them


def corpus(limit, per_file):
    from chunk_zpack_bench import usr_lib_files
    files, _ = usr_lib_files(1 << 40)
    pieces, names, total = [], [], 0
    for path, _ in files:
        if total >= limit:
            break
        with open(path, "rb") as f:
            data = f.read(min(per_file, limit - total))
        names.append((path, len(data)))
        total += len(data)
        pieces += [data[i:i + PIECE] for i in range(0, len(data), PIECE)]
    return pieces, names, total


def main():
    import zpack_cases as zc
    import zpack2_cases as z2
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zpack_l2_model.txt")
    limit = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000
    per_file = int(float(sys.argv[3])) if len(sys.argv) > 3 else 262144
    pieces, names, total = corpus(limit, per_file)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("zpack level 2, the model's ratio (tools/zpack_model_ratio.py %d %d): %d bytes in %d pieces of %d, the first %d bytes of each of"
        % (limit, per_file, total, len(pieces), PIECE, per_file))
    for path, n in names:
        say("        %9d  %s" % (n, path))
    yard = sum(len(zlib.compress(p, 1)) for p in pieces)
    t0 = time.perf_counter()
    one = sum(len(zc.compress_chunk(p)) for p in pieces)
    say("%-44s %10s %9s %9s %9s" % ("parse", "stored", "/ input", "/ level 1", "/ zlib -1"))
    say("%-44s %10d %9.4f %9.4f %9.4f" % ("zlib.compress(piece, 1)", yard, yard / total, yard / one, 1.0))
    say("%-44s %10d %9.4f %9.4f %9.4f   (%.0f s)" % ("level 1 (zpack_cases.parse)", one, one / total, 1.0, one / yard, time.perf_counter() - t0))
    off = dict((e, False) for e in ELEMENTS)
    rows = [("level 2's frame, no element: level 1 again", dict(off))]
    rows += [("only (%s) %s" % (LETTER[e], e), dict(off, **{e: True})) for e in ELEMENTS]
    rows += [("all but (%s) %s" % (LETTER[e], e), dict((k, k != e) for k in ELEMENTS)) for e in ELEMENTS]
    rows += [("level 2: (a) (b) (c) (d) and backwards", dict((e, True) for e in ELEMENTS))]
    for name, kw in rows:
        t0 = time.perf_counter()
        stored = 0
        for p in pieces:
            s = z2.compress_chunk2(p, **kw)
            if len(s) < len(p):
                assert zc.lz4_block_decode(s, len(p)) == p
            stored += len(s)
        say("%-44s %10d %9.4f %9.4f %9.4f   (%.0f s)" % (name, stored, stored / total, stored / one, stored / yard, time.perf_counter() - t0))
        if not any(kw.values()):
            assert stored == one, "the frame without an element is level 1's parse"
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
