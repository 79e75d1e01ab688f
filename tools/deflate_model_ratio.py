"""The device deflate leg, measured ON THE MODEL (writes profiles/gzip_device_model.txt).  CPU only.

The blob is a property of the model, which the kernels reproduce byte for byte, so the ratio is settled here.  The corpus is
that of profiles/chunk_zentropy_model.txt (tools/zpack_model_ratio.py's: regular files under /usr/lib, largest first, the first
`per_file` bytes of each), taken as ONE stream.  The model's blob (pieces of 65 536 bytes) is held against what the host leg writes
for the same stream at level 1 and at the default level -- 1 MiB blocks, each a raw deflate stream closed with a sync flush, the
same construction (without the host leg's probe for incompressible blocks, which stores them) -- and against the zpack entropy
stage's "level 1 + stage" on the same bytes in its own pieces of 8 192.  Every piece's form is inflated again by zlib and must give
its bytes: that is asserted.  No ratio is.
deflate_model_ratio.py [out = profiles/gzip_device_model.txt] [bytes = 3e6] [per_file = 262144]"""
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def host_leg(stream, level):
    out = 0
    for at in range(0, len(stream), 1 << 20):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
        out += len(z.compress(stream[at:at + (1 << 20)]) + z.flush(zlib.Z_SYNC_FLUSH))
    return out


def main():
    import deflate_cases as dc
    import zentropy_cases as ze
    from zpack_model_ratio import corpus
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "gzip_device_model.txt")
    limit = int(float(sys.argv[2])) if len(sys.argv) > 2 else 3_000_000
    per_file = int(float(sys.argv[3])) if len(sys.argv) > 3 else 262144
    pieces8k, names, total = corpus(limit, per_file)
    stream = b"".join(bytes(p) for p in pieces8k)
    assert len(stream) == total
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device deflate leg, the model's ratio (tools/deflate_model_ratio.py %d %d): one stream of %d bytes, the first %d bytes of each of"
        % (limit, per_file, total, per_file))
    for path, n in names:
        say("        %9d  %s" % (n, path))
    t0 = time.perf_counter()
    stored = n_dyn = n_pieces = 0
    for at in range(0, total, dc.PIECE):
        piece = stream[at:at + dc.PIECE]
        plan = dc.piece_plan(piece)
        form = dc.dynamic_form(plan) if plan["dynamic"] else dc.stored_form(piece)
        d = zlib.decompressobj(-15)
        assert d.decompress(form + b"\x03\x00") == piece and d.eof, "piece %d does not inflate to its bytes" % (at // dc.PIECE)
        stored += len(form)
        n_dyn += plan["dynamic"]
        n_pieces += 1
    assert dc.inflate(dc.deflate_blob(stream[:3 * dc.PIECE + 5])) == stream[:3 * dc.PIECE + 5]
    say("(the model over %d pieces, every form inflated again by zlib: %.0f s)" % (n_pieces, time.perf_counter() - t0))
    l1, l6 = host_leg(stream, 1), host_leg(stream, -1)
    t0 = time.perf_counter()
    staged = 0
    for p in pieces8k:
        u = ze.under_form(p, 1)
        h = ze.huff_size(u, ze.STREAMS, ze.MAX_BITS)
        staged += h if h < len(u) - (len(u) >> 4) else len(u)
    say("(level 1 + stage over %d pieces of 8192: %.0f s)" % (len(pieces8k), time.perf_counter() - t0))
    say("%-66s %10s %9s %9s %9s" % ("form", "stored", "/ input", "/ host 1", "/ host -1"))

    def row(name, v):
        say("%-66s %10d %9.4f %9.4f %9.4f" % (name, v, v / total, v / l1, v / l6))
    row("host leg, level 1 (1 MiB blocks, sync-flushed)", l1)
    row("host leg, default level", l6)
    row("device leg: the model (%d pieces, %d dynamic, %d stored)" % (n_pieces, n_dyn, n_pieces - n_dyn), stored)
    row("zpack level 1 + stage, 32 streams (pieces of 8 192; DESIGN 4.16)", staged)
    if stored < staged:
        say("the device leg stores fewer bytes than level 1 + stage: %d < %d" % (stored, staged))
    else:
        say("THE DEVICE LEG DOES NOT STORE FEWER BYTES THAN LEVEL 1 + STAGE: %d >= %d" % (stored, staged))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
