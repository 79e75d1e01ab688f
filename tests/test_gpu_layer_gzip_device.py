"""GPU tests of the layer writer's device gzip leg (mi_layer_set_gzip_ctx, MI_MEMFS_GZIP_DEVICE): the blob is the
ten header bytes, the model of the tar (deflate_cases.py), 03 00, the CRC and the length; it inflates to the tar the same layer
writes with MI_GZIP_OFF; TarDigest is the host leg's; gzip_sha256 is the SHA-256 of the file written; the window does not show;
an empty layer; the commit option on one ctx and over two ctxs on one device; one scenario under MI_GUARD_ALLOC=1 in a process
of its own, the last piece ending on the allocation's last byte (no positive control: a deliberate fault has no place here)."""
import gzip
import hashlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import deflate_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


FILES = (("a/text.txt", lambda: dc.text(300000, 31)), ("a/zeros.bin", lambda: bytes(1 << 20)), ("b/random.bin", lambda: dc.random_bytes(700000, 32)),
         ("b/spans.dat", lambda: dc.symbols(1091456, 16, 33)), ("c/small", lambda: b"hello\n"))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """about 3 MiB + 700 bytes of mixed files (text, zeros, random, a file spanning two blocks)"""
    root = tmp_path_factory.mktemp("gzdev") / "root"
    for rel, make in FILES:
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(make())
        os.utime(p, (1700000000, 1700000000))
    for d in ("a", "b", "c", ""):
        os.utime(root / d, (1700000000, 1700000000))
    return str(root)


def _entries(root):
    return M.tree_walk(root, root, (), M.TREE_SCAN, full=True)


def _write(root, path, gzip_level, engine=None, entries=None):
    ents = _entries(root) if entries is None else entries
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    l = M.Layer(out_fd=fd, gzip_level=gzip_level)
    try:
        if engine is not None:
            l.set_gzip_engine(engine)
        for e in ents:
            l.add(e, os.path.join(root, e["relpath"].lstrip("/")) if e["kind"] == 1 else None)
        return l.finish()
    finally:
        l.close()
        os.close(fd)


@pytest.fixture(scope="module")
def reference(tree, tmp_path_factory):
    """the tar (MI_GZIP_OFF), the host leg's result and the model's member, computed once"""
    d = tmp_path_factory.mktemp("gzref")
    off = _write(tree, str(d / "layer.tar"), M.GZIP_OFF)
    tar = open(d / "layer.tar", "rb").read()
    host = _write(tree, str(d / "host.gz"), M.GZIP_DEFAULT)
    assert 3 * (1 << 20) < len(tar) < 3 * (1 << 20) + 200000 and gzip.decompress(open(d / "host.gz", "rb").read()) == tar
    return dict(tar=tar, off=off, host=host, member=dc.gzip_member(tar))


@pytest.mark.parametrize("window", ["1", None])
@pytest.mark.parametrize("level", [M.GZIP_DEFAULT, 1, 9])
def test_the_blob_is_the_models_member_whatever_the_window_and_the_level(engine, tree, reference, tmp_path, monkeypatch, window, level):
    if window:
        monkeypatch.setenv("MI_GZIP_DEVICE_WINDOW_MB", window)
    else:
        monkeypatch.delenv("MI_GZIP_DEVICE_WINDOW_MB", raising=False)
    res = _write(tree, str(tmp_path / "dev.gz"), level, engine)
    blob = open(tmp_path / "dev.gz", "rb").read()
    tar = reference["tar"]
    assert blob[:10] == bytes((0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 4, 255))
    assert blob[-10:-8] == b"\x03\x00" and blob[-8:] == (zlib.crc32(tar)).to_bytes(4, "little") + (len(tar) & 0xFFFFFFFF).to_bytes(4, "little")
    assert blob == reference["member"]
    assert gzip.decompress(blob) == tar
    assert res["tar_sha256"] == reference["host"]["tar_sha256"] == reference["off"]["tar_sha256"] == hashlib.sha256(tar).digest()
    assert res["gzip_sha256"] == hashlib.sha256(blob).digest() and res["gzip_bytes"] == len(blob) and res["tar_bytes"] == len(tar)
    assert res["n_entries"] == reference["host"]["n_entries"]


def test_an_empty_layer(engine, tmp_path):
    path = str(tmp_path / "empty.gz")
    fd = os.open(path, os.O_WRONLY | os.O_CREAT, 0o644)
    l = M.Layer(out_fd=fd, gzip_level=M.GZIP_DEFAULT)
    try:
        l.set_gzip_engine(engine)
        with pytest.raises(M.MiError) as ei:
            l.set_gzip_engine(engine)                                    # once
        assert ei.value.code == -6
        res = l.finish()
    finally:
        l.close()
        os.close(fd)
    blob = open(path, "rb").read()
    assert blob == dc.gzip_member(bytes(1024)) and gzip.decompress(blob) == bytes(1024)
    assert res["gzip_sha256"] == hashlib.sha256(blob).digest() and res["tar_sha256"] == hashlib.sha256(bytes(1024)).digest()


def _commit(root, tmp_path, name, engine, gzip_level, device):
    path = str(tmp_path / name)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        with M.MemFS(root) as fs:
            if device:
                fs.set_options(gzip_device=True)
            res = fs.commit_layer(must_scan=True, out_fd=fd, gzip_level=gzip_level, engine=engine)
    finally:
        os.close(fd)
    return res, open(path, "rb").read()


def _layer_key(res):
    return [(e["relpath"], e["kind"], e["size"], bytes(e.get("root") or b"")) for e in res["layer"]]


def test_the_commit_option_on_one_ctx_and_over_two_ctxs_on_one_device(engine, tree, tmp_path):
    # the tar of this commit (its layer has no entry for the root itself): without the option, at MI_GZIP_OFF
    off_plain, tar = _commit(tree, tmp_path, "off_plain.tar", engine, M.GZIP_OFF, False)
    assert hashlib.sha256(tar).hexdigest() in str(off_plain["tar_digest"]) and len(tar) > 3 * (1 << 20)
    member = dc.gzip_member(tar)
    plain, plain_blob = _commit(tree, tmp_path, "plain.gz", engine, M.GZIP_DEFAULT, False)
    one, one_blob = _commit(tree, tmp_path, "one.gz", engine, M.GZIP_DEFAULT, True)
    with M.Engine(device=0, n_streams=4) as second:
        two, two_blob = _commit(tree, tmp_path, "two.gz", [engine, second], M.GZIP_DEFAULT, True)
        two_plain, _ = _commit(tree, tmp_path, "two_plain.gz", [engine, second], M.GZIP_DEFAULT, False)
    assert gzip.decompress(plain_blob) == tar and plain["tar_digest"] == two_plain["tar_digest"] == off_plain["tar_digest"]
    for res, blob in ((one, one_blob), (two, two_blob)):
        assert _layer_key(res) == _layer_key(plain) and any(k[3] for k in _layer_key(res))          # entries and roots
        assert res["tar_digest"] == plain["tar_digest"] and res["tar_bytes"] == len(tar)
        assert blob == member and gzip.decompress(blob) == tar
        assert res["gzip_bytes"] == len(blob) and str(res["gzip_digest"]).endswith(hashlib.sha256(blob).hexdigest())
    assert plain_blob != one_blob
    # no effect at MI_GZIP_OFF
    off, off_blob = _commit(tree, tmp_path, "off.tar", engine, M.GZIP_OFF, True)
    assert off_blob == tar and off["tar_digest"] == off_plain["tar_digest"] and _layer_key(off) == _layer_key(plain)


GUARDED = r'''
import sys, zlib
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import makisu_amd as M
import deflate_cases as dc
data = dc.text(65536 + 4096, 41)            # a multiple of 256: the input's allocation ends with the last piece's last byte
with M.Engine(device=0) as eng:
    blob, crc, info = eng.deflate_buffer(data)
    assert blob == dc.deflate_blob(data) and crc == zlib.crc32(data) and info["n_pieces"] == 2, info
    r = dc.random_bytes(65536 + 256, 42)    # ... and as stored blocks
    blob, crc, info = eng.deflate_buffer(r)
    assert blob == dc.deflate_blob(r) and crc == zlib.crc32(r) and info["n_stored"] == 2, info
print("OK")
'''


def test_no_read_leaves_the_input_under_the_guard():
    env = dict(os.environ, MI_GUARD_ALLOC="1")
    p = subprocess.run([sys.executable, "-c", GUARDED % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr[-3000:]
