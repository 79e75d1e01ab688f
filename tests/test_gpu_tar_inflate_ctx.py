"""GPU tests of mi_tar_inflate_ctx (Engine.tar_inflate): mi_tar_inflate's contract and results through the device -- the
reference's Go-written fixture blob (a foreign single-stream blob, one wave), layers of both of this library's writers, the
fallback to the host path for a blob that is not parallel, a plain tar, a corrupt blob."""
import base64
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import makisu_amd as M  # noqa: E402
import deflate_cases as dc  # noqa: E402
import inflate_cases as ic  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
GO_LAYER_TAR_DIGEST = "4ac76077f2c741c856a2419dfdb0804b18e48d2e1a9ce9c6a3f0605a2078caba"


@pytest.fixture(scope="module")
def engine():
    with M.Engine(device=0) as e:
        yield e


def _same(engine, blob_path, tmp_path, fell_back):
    """both calls on one blob, with and without an output file: the same results, the same tar"""
    host = M.tar_inflate(str(blob_path), str(tmp_path / "host.tar"))
    dev = engine.tar_inflate(str(blob_path), str(tmp_path / "dev.tar"))
    info = dev.pop("info")
    assert dev == host and info["fell_back"] == fell_back, (dev, host, info)
    tar = (tmp_path / "dev.tar").read_bytes()
    assert tar == (tmp_path / "host.tar").read_bytes() and len(tar) == dev["tar_bytes"]
    assert dev["tar_digest"] == "sha256:" + hashlib.sha256(tar).hexdigest()
    assert dev["blob_digest"] == "sha256:" + hashlib.sha256(open(blob_path, "rb").read()).hexdigest()
    only = engine.tar_inflate(str(blob_path))                            # digests only
    assert only.pop("info")["fell_back"] == fell_back and only == host
    return tar, info


def test_the_references_fixture_blob_through_the_device(engine, tmp_path):
    blob_path = tmp_path / "blob"
    blob_path.write_bytes(base64.b64decode(json.load(open(os.path.join(GOLDEN, "sha256_reference_fixtures.json")))["vectors"][0]["file_b64"]))
    tar, info = _same(engine, blob_path, tmp_path, 0)
    assert len(tar) == 1308672 and "sha256:" + hashlib.sha256(tar).hexdigest() == "sha256:" + GO_LAYER_TAR_DIGEST
    assert info["verdict"] == M.INFLATE_DONE and info["n_segments"] >= 1 and info["out_bytes"] == 1308672


def _layer(root, path, engine=None):
    ents = M.tree_walk(root, root, (), M.TREE_SCAN, full=True)
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    l = M.Layer(out_fd=fd, gzip_level=M.GZIP_DEFAULT)
    try:
        if engine is not None:
            l.set_gzip_engine(engine)
        for e in ents:
            l.add(e, os.path.join(root, e["relpath"].lstrip("/")) if e["kind"] == 1 else None)
        return l.finish()
    finally:
        l.close()
        os.close(fd)


def test_layers_of_both_writers(engine, tmp_path):
    root = tmp_path / "root"
    for rel, data in (("a/text.txt", dc.text(300000, 81)), ("a/zeros.bin", bytes(1 << 20)), ("b/random.bin", dc.random_bytes(200000, 82)),
                      ("c/small", b"hello\n")):
        (root / rel).parent.mkdir(parents=True, exist_ok=True)
        (root / rel).write_bytes(data)
    for leg, eng in (("device", engine), ("host", None)):
        d = tmp_path / leg
        d.mkdir()
        res = _layer(str(root), str(d / "layer.gz"), eng)
        tar, info = _same(engine, d / "layer.gz", d, 0)
        assert info["verdict"] == M.INFLATE_DONE and info["n_segments"] >= 2 and len(tar) == res["tar_bytes"]
        assert res["tar_sha256"] == hashlib.sha256(tar).digest()


def test_a_blob_that_is_not_parallel_goes_through_the_host_path(engine, tmp_path):
    data = dc.text(140000, 64)
    blob = tmp_path / "noreset.gz"
    blob.write_bytes(ic.no_reset(data))
    tar, info = _same(engine, blob, tmp_path, 1)
    assert tar == data and info["verdict"] == M.INFLATE_NOT_PARALLEL and info["rule"] == ic.DISTANCE


def test_a_plain_tar_is_copied_and_a_corrupt_blob_leaves_no_file(engine, tmp_path):
    plain = tmp_path / "plain.tar"
    plain.write_bytes(dc.text(10240, 83))
    tar, info = _same(engine, plain, tmp_path, 0)
    assert tar == plain.read_bytes() and info["n_segments"] == 0
    gz, _ = ic.two_piece()
    bad = tmp_path / "bad.gz"
    for name, m in (("a broken rule", gz[:-100]), ("a wrong CRC", gz[:-8] + bytes((gz[-8] ^ 1,)) + gz[-7:])):
        assert ic.zlib_inflates(m) is None and ic.plan(m)["result"] == ic.INVALID
        bad.write_bytes(m)
        out = tmp_path / "bad.tar"
        with pytest.raises(M.MiError) as ei:
            engine.tar_inflate(str(bad), str(out))
        assert ei.value.code == -1 and str(bad) + ": corrupt gzip stream" in str(ei.value), (name, ei.value)
        assert not out.exists(), name
        with pytest.raises(M.MiError) as eh:
            M.tar_inflate(str(bad))
        assert str(bad) + ": " in str(eh.value) and ("gzip stream" in str(eh.value))   # the host path's kind of text: the blob, then what is wrong
    assert engine.tar_inflate(str(plain))["tar_bytes"] == 10240                    # the ctx stays usable
