"""mi_zset_recode's ratio, measured ON THE MODEL (writes profiles/chunk_zrecode_model.txt).  CPU only.

The stored bytes are a property of the rule, and the kernels reproduce the model byte for byte, so the ratio is settled here.
The corpus is that of tools/zpack_model_ratio.py (profiles/chunk_zpack_l2_model.txt): regular files under /usr/lib of the box,
largest first, the first `per_file` bytes of each until `bytes` are read, cut in 8 KiB pieces.  Every piece is coded by level 1's
model; tests/zrecode_cases.recode_form then recodes that form at level 2 (level 1 -> level 2) and, the other way round, level
2's form at level 1.  By the rule the sum afterwards is at most the smaller of the two levels' sums.
zrecode_model_ratio.py [out = profiles/chunk_zrecode_model.txt] [bytes = 3e6] [per_file = 262144]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import zrecode_cases as rc
    from zpack_model_ratio import PIECE, corpus
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_zrecode_model.txt")
    limit = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000
    per_file = int(float(sys.argv[3])) if len(sys.argv) > 3 else 262144
    pieces, names, total = corpus(limit, per_file)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("mi_zset_recode, the model's ratio (tools/zrecode_model_ratio.py %d %d): %d bytes in %d pieces of %d, the corpus of "
        "profiles/chunk_zpack_l2_model.txt (%d files under /usr/lib, the first %d bytes of each)" % (limit, per_file, total, len(pieces), PIECE, len(names), per_file))
    one = [rc.coded(p, 1) for p in pieces]
    two = [rc.coded(p, 2) for p in pieces]
    s1, s2 = sum(map(len, one)), sum(map(len, two))
    say("%-52s %10s %14s" % ("held", "stored", "/ stored before"))
    say("%-52s %10d" % ("level 1's forms", s1))
    say("%-52s %10d %14.4f" % ("level 2's forms (mi_pack_compress, every chunk)", s2, s2 / s1))
    for name, src, level, before in (("level 1's forms recoded at level 2", one, 2, s1), ("level 2's forms recoded at level 1", two, 1, s2)):
        after = [rc.recode_form(f, len(p), level) for f, p in zip(src, pieces)]
        for f, p in zip(after, pieces):
            assert rc.plain_of(f, len(p)) == p
        n = sum(1 for a, b in zip(after, src) if a != b)
        say("%-52s %10d %14.4f   %d of %d forms replaced" % (name, sum(map(len, after)), sum(map(len, after)) / before, n, len(pieces)))
    both = sum(min(len(a), len(b)) for a, b in zip(one, two))
    grew = sum(1 for a, b in zip(one, two) if len(b) > len(a))
    say("%-52s %10d %14.4f   level 2 stores MORE for %d of %d pieces" % ("the smaller of the two forms, piece by piece", both, both / s1, grew, len(pieces)))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
