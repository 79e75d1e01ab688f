"""CPU tests of the layer-tar reader (csrc/mi_tar.hip, no GPU): entries and file byte ranges of
ustar / pax / GNU archives against Python's tarfile (an independent implementation of the same
formats), plus the reference's own docker-made layer fixture (testdata/files/busybox/.../layer.tar, SURVEY.md 8c: the gunzip
of the stored layer blob that tests/golden/sha256_reference_fixtures.json carries)."""
import hashlib
import io
import os
import posixpath
import tarfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _reference_fixtures(tmp_path):
    """(the reference's stored layer blob testdata/files/alpine/test_layer.tar, its gunzip testdata/files/busybox/393ccd5c.../
    layer.tar) as files under tmp_path, from the blob in tests/golden/sha256_reference_fixtures.json"""
    import base64
    import json
    import zlib
    vec = json.load(open(os.path.join(GOLDEN, "sha256_reference_fixtures.json")))["vectors"][0]
    assert vec["name"] == "alpine_layer_blob"
    blob = base64.b64decode(vec["file_b64"])
    assert hashlib.sha256(blob).hexdigest() == GZ_BLOB_SHA
    d = tmp_path / "reference_fixtures"
    d.mkdir(exist_ok=True)
    gz_path, tar_path = str(d / "test_layer.tar"), str(d / "layer.tar")
    open(gz_path, "wb").write(blob)
    open(tar_path, "wb").write(zlib.decompress(blob, 31))
    return gz_path, tar_path


def _rel(name):
    n = posixpath.normpath("/" + name).lstrip("/")
    return n or "."


def _kind(m):
    if m.isdir():
        return 0
    if m.isreg():
        return 1
    if m.issym():
        return 2
    if m.islnk():
        return 3
    return 4


def _compare_with_tarfile(path):
    import makisu_amd
    got = makisu_amd.tar_entries(path)
    with tarfile.open(path) as tf:
        members = tf.getmembers()
        assert len(got) == len(members)
        n_reg = 0
        raw = open(path, "rb")
        for g, m in zip(got, members):
            assert g["relpath"] == _rel(m.name), m.name
            assert g["kind"] == _kind(m), m.name
            assert g["mode"] & 0o7777 == m.mode & 0o7777 and g["uid"] == m.uid and g["gid"] == m.gid
            assert g["mtime_sec"] == int(m.mtime // 1), m.name
            if m.issym() or m.islnk():
                assert g["link_target"] == m.linkname
            else:
                assert g["link_target"] is None
            if m.isreg():
                assert g["size"] == m.size and g["file_index"] == n_reg
                assert g["data_offset"] == m.offset_data
                raw.seek(g["data_offset"])
                assert hashlib.sha256(raw.read(g["size"])).digest() == \
                    hashlib.sha256(tf.extractfile(m).read()).digest()
                n_reg += 1
            else:
                assert g["size"] == 0 and g["file_index"] == -1
        raw.close()
    return got


def _build(path, fmt):
    long_dir = "d" * 60 + "/" + "e" * 70 + "/" + "f" * 90                 # > 100: prefix / long name
    very_long = "v" * 200 + "/" + "w" * 120 + "/file"                      # > 255 in total: pax path / GNU 'L'
    with tarfile.open(path, "w", format=fmt) as tf:
        def add(name, type_=tarfile.REGTYPE, data=b"", **kw):
            ti = tarfile.TarInfo(name)
            ti.type = type_
            ti.size = len(data)
            ti.mode = kw.get("mode", 0o644)
            ti.uid, ti.gid = kw.get("uid", 0), kw.get("gid", 0)
            ti.mtime = kw.get("mtime", 1494882420)
            ti.linkname = kw.get("linkname", "")
            ti.uname = ti.gname = ""
            ti.devmajor, ti.devminor = kw.get("dev", (0, 0))
            tf.addfile(ti, io.BytesIO(data) if data else None)
        add("./", tarfile.DIRTYPE, mode=0o755)
        add("bin/", tarfile.DIRTYPE, mode=0o755)
        add("bin/busybox", data=os.urandom(70001), mode=0o755)
        add("bin/sh", tarfile.LNKTYPE, linkname="bin/busybox", mode=0o755)          # hard link
        add("bin/link", tarfile.SYMTYPE, linkname="/bin/busybox", mode=0o777)
        add("etc/", tarfile.DIRTYPE, mode=0o755)                                     # (directories their owner can enter)
        add("etc/empty")
        add("etc/one", data=b"x")
        add("etc/block512", data=bytes(512))                                          # exactly one block
        add("etc/.wh.removed")                                                        # a whiteout marker
        add("dev/null", tarfile.CHRTYPE, dev=(1, 3), mode=0o666)
        add("dev/fifo", tarfile.FIFOTYPE)
        add(long_dir + "/", tarfile.DIRTYPE, mode=0o755)
        add(long_dir + "/payload", data=b"long path payload", uid=1000, gid=2000)
        add("owner", data=b"o", uid=123456, gid=654321, mtime=1)
        if fmt != tarfile.USTAR_FORMAT:
            add(very_long, data=b"very long")
            add("sym-long", tarfile.SYMTYPE, linkname="t" * 200)                     # > 100: linkpath / 'K'
            add("café/üml", data=b"utf8")
            add("big-ids", data=b"b", uid=3000000, gid=4000000)                       # > 7 octal digits
    return path


@pytest.mark.parametrize("fmt", [tarfile.USTAR_FORMAT, tarfile.PAX_FORMAT, tarfile.GNU_FORMAT])
def test_tar_entries_match_tarfile(tmp_path, fmt):
    got = _compare_with_tarfile(_build(str(tmp_path / "layer.tar"), fmt))
    by = {g["relpath"]: g for g in got}
    assert got[0]["relpath"] == "." and got[0]["kind"] == 0
    assert by["bin/sh"]["kind"] == 3 and by["bin/sh"]["link_target"] == "bin/busybox"
    assert by["bin/link"]["link_target"] == "/bin/busybox"
    assert by["dev/null"]["kind"] == 4 and by["dev/fifo"]["kind"] == 4
    assert by["etc/.wh.removed"]["kind"] == 1 and by["etc/.wh.removed"]["size"] == 0
    assert by["etc/block512"]["data_offset"] % 512 == 0
    regs = [g for g in got if g["kind"] == 1]
    assert [g["file_index"] for g in regs] == list(range(len(regs)))


def test_tar_pax_mtime_fraction_and_errors(tmp_path):
    import makisu_amd
    p = str(tmp_path / "frac.tar")
    with tarfile.open(p, "w", format=tarfile.PAX_FORMAT) as tf:
        ti = tarfile.TarInfo("a")
        ti.mtime = 1494882420.75                       # pax carries the fraction; entries hold whole seconds
        tf.addfile(ti)
    assert makisu_amd.tar_entries(p)[0]["mtime_sec"] == 1494882420
    # an empty archive (two zero blocks, what Go's tar.Writer writes on Close) has no entries
    empty = str(tmp_path / "empty.tar")
    open(empty, "wb").write(bytes(1024))
    assert makisu_amd.tar_entries(empty) == []
    # a flipped header byte fails the checksum; a truncated member is reported, not read past
    raw = bytearray(open(_build(str(tmp_path / "ok.tar"), tarfile.USTAR_FORMAT), "rb").read())
    bad = bytearray(raw)
    bad[512 + 3] ^= 0x20
    open(str(tmp_path / "bad.tar"), "wb").write(bad)
    with pytest.raises(makisu_amd.MiError) as ei:
        makisu_amd.tar_entries(str(tmp_path / "bad.tar"))
    assert ei.value.code == -1
    open(str(tmp_path / "cut.tar"), "wb").write(raw[: 3 * 512 + 1000])      # inside bin/busybox's data
    with pytest.raises(makisu_amd.MiError):
        makisu_amd.tar_entries(str(tmp_path / "cut.tar"))
    with pytest.raises(makisu_amd.MiError) as ei:
        makisu_amd.tar_entries(str(tmp_path / "missing.tar"))
    assert ei.value.code == -5


def test_reference_layer_fixture(tmp_path):
    """The reference's docker-made busybox layer (390 entries, one binary and its hard links)."""
    _, fixture = _reference_fixtures(tmp_path)
    assert hashlib.sha256(open(fixture, "rb").read()).hexdigest() == GZ_TAR_SHA
    got = _compare_with_tarfile(fixture)
    assert len(got) == 390
    kinds = [g["kind"] for g in got]
    assert kinds.count(3) > 300 and kinds.count(1) >= 1
    big = max(got, key=lambda g: g["size"])
    assert big["relpath"] == "bin/[" and big["size"] == 1026712


def test_tar_entries_feed_the_snapshot_diff(tmp_path):
    """A layer tar as the 'before' side: extract it, edit the tree, walk, diff."""
    import makisu_amd
    p = _build(str(tmp_path / "layer.tar"), tarfile.GNU_FORMAT)
    before = [e for e in makisu_amd.tar_entries(p) if e["kind"] in (0, 1, 2)]
    root = tmp_path / "fs"
    with tarfile.open(p) as tf:
        members = [m for m in tf.getmembers() if m.isdir() or m.isreg() or m.issym()]
        tf.extractall(root, members=members)
    # the archive's absolute symlink means "inside the image root": on disk under `root` it has to
    # point there, and the scan walk trims the root off again (createHeader's TrimRoot)
    os.unlink(root / "bin" / "link")
    os.symlink(str(root) + "/bin/busybox", root / "bin" / "link")
    for m in members:                                    # extraction order leaves directory mtimes bumped
        os.utime(root / m.name, (m.mtime, m.mtime), follow_symlinks=False)
    after = makisu_amd.tree_walk(str(root), rel_base=str(root), mode=makisu_amd.TREE_SCAN, full=True)
    for e in after:                                      # we are not root here: owners differ from the archive's
        e["uid"] = e["gid"] = 0
    for e in before:
        e["uid"] = e["gid"] = 0
    flags, wh = makisu_amd.snapshot_diff(before, after)
    changed = sorted(e["relpath"] for e, f in zip(after, flags) if f == makisu_amd.DIFF_CHANGED)
    # the only "new" paths are parent directories the archive never listed (tar allows that)
    known = {e["relpath"] for e in before}
    implied = sorted(e["relpath"] for e in after if e["relpath"] not in known)
    assert implied and all(e["kind"] == 0 for e in after if e["relpath"] in implied)
    assert changed == implied and not any(wh), changed
    (root / "etc" / "one").write_bytes(b"xy")
    os.unlink(root / "bin" / "link")
    after = makisu_amd.tree_walk(str(root), rel_base=str(root), mode=makisu_amd.TREE_SCAN, full=True)
    for e in after:
        e["uid"] = e["gid"] = 0
    flags, wh = makisu_amd.snapshot_diff(before, after, ignore_time=True)
    assert sorted(e["relpath"] for e, f in zip(after, flags)
                  if f == makisu_amd.DIFF_CHANGED and e["relpath"] in known) == ["etc/one"]
    assert [e["relpath"] for e, w in zip(before, wh) if w] == ["bin/link"]


def _layer_tar(path, items):
    """items: (name, kind, data_or_link, mtime) with kind 'd' / 'f' / 'l'."""
    with tarfile.open(path, "w", format=tarfile.GNU_FORMAT) as tf:
        for name, kind, payload, mtime in items:
            ti = tarfile.TarInfo(name)
            ti.mtime = mtime
            ti.uname = ti.gname = ""
            if kind == "d":
                ti.type, ti.mode = tarfile.DIRTYPE, 0o755
                tf.addfile(ti)
            elif kind == "l":
                ti.type, ti.mode, ti.linkname = tarfile.SYMTYPE, 0o777, payload
                tf.addfile(ti)
            else:
                ti.size, ti.mode = len(payload), 0o644
                tf.addfile(ti, io.BytesIO(payload))
    return path


def _extract_like_untar_one_item(root, tar_path):
    """Independent emulation of untarOneItem on a real directory: whiteouts delete, dir-on-dir keeps
    children, everything else replaces (RemoveAll + recreate)."""
    import shutil
    with tarfile.open(tar_path) as tf:
        for m in tf.getmembers():
            dst = os.path.join(root, m.name)
            base = os.path.basename(m.name.rstrip("/"))
            if base.startswith(".wh."):
                victim = os.path.join(os.path.dirname(dst.rstrip("/")), base[4:])
                if os.path.islink(victim) or os.path.isfile(victim):
                    os.unlink(victim)
                elif os.path.isdir(victim):
                    shutil.rmtree(victim)
                continue
            if os.path.lexists(dst):
                if m.isdir() and os.path.isdir(dst) and not os.path.islink(dst):
                    continue
                if os.path.isdir(dst) and not os.path.islink(dst):
                    shutil.rmtree(dst)
                else:
                    os.unlink(dst)
            if m.isdir():
                os.makedirs(dst)
            elif m.issym():
                os.symlink(m.linkname, dst)
            else:
                with open(dst, "wb") as f:
                    f.write(tf.extractfile(m).read())


def test_apply_layer_matches_sequential_extraction(tmp_path):
    """The layer merge (mi_memfs_update_from_entries, through makisu_amd.apply_layer) over three layer tars == the
    paths (and kinds, sizes) left on disk after extracting the same tars in order with untarOneItem's rules."""
    import makisu_amd
    t = 1500000000
    l1 = _layer_tar(str(tmp_path / "l1.tar"), [
        ("etc/", "d", None, t), ("etc/passwd", "f", b"root\n", t), ("etc/conf.d/", "d", None, t),
        ("etc/conf.d/a", "f", b"a", t), ("etc/conf.d/b", "f", b"b", t), ("usr/", "d", None, t),
        ("usr/bin/", "d", None, t), ("usr/bin/tool", "f", b"v1", t), ("usr/share/", "d", None, t),
        ("usr/share/doc/", "d", None, t), ("usr/share/doc/readme", "f", b"r", t), ("link", "l", "etc/passwd", t)])
    l2 = _layer_tar(str(tmp_path / "l2.tar"), [
        ("etc/", "d", None, t + 5),                                   # dir on dir: children stay
        ("etc/passwd", "f", b"root\nme\n", t + 5),                    # replaced (size differs)
        ("etc/conf.d/.wh.a", "f", b"", t + 5),                        # whiteout of a file
        ("usr/share/.wh.doc", "f", b"", t + 5),                       # whiteout of a subtree
        ("usr/bin/tool", "f", b"v2", t),                              # similar header (same size, mtime): stays OLD
        ("link", "d", None, t + 5),                                   # symlink replaced by a directory
        ("link/inside", "f", b"i", t + 5)])
    l3 = _layer_tar(str(tmp_path / "l3.tar"), [
        ("etc/conf.d", "f", b"now a file", t + 9),                    # directory replaced by a file: subtree goes
        ("usr/share/doc/", "d", None, t + 9), ("usr/share/doc/new", "f", b"n", t + 9),   # deleted path comes back
        (".wh.link", "f", b"", t + 9)])                               # top-level whiteout
    root = tmp_path / "fs"
    os.makedirs(root)
    tree = []
    for tar_path in (l1, l2, l3):
        layer = makisu_amd.tar_entries(tar_path)
        tree = makisu_amd.apply_layer(tree, layer)
        _extract_like_untar_one_item(str(root), tar_path)
        on_disk = {}
        for dp, dns, fns in os.walk(root):
            for n in dns + fns:
                full = os.path.join(dp, n)
                st = os.lstat(full)
                kind = 2 if os.path.islink(full) else (0 if os.path.isdir(full) else 1)
                on_disk[os.path.relpath(full, root)] = (kind, st.st_size if kind == 1 else 0)
        got = {e["relpath"]: (e["kind"], e["size"]) for e in tree if e["relpath"] != "."}
        assert got == on_disk, tar_path
        rels = [e["relpath"] for e in tree]
        assert rels == sorted(rels, key=lambda r: ("/" if r == "." else "/" + r).encode())
    final = {e["relpath"]: e for e in tree}
    assert "link" not in final and "etc/conf.d/b" not in final and final["etc/conf.d"]["kind"] == 1
    assert final["usr/share/doc/new"]["size"] == 1
    # (the "similar header" quirk -- layer 2's usr/bin/tool does NOT replace layer 1's entry -- shows in nothing the tree
    # keeps: test_hard_links_are_applied_after_everything_else holds "the OLD entry stays" on a field that differs)


# ---- round 2: stored (gzip) layers, UpdateFromTarReader's filter, hard-link pass, isOnDisk ----
import makisu_amd as M  # noqa: E402

GZ_BLOB_SHA = "393ccd5c4dd90344c9d725125e13f636ce0087c62f5ca89050faaacbb9e3ed5b"   # testutil.SampleLayerTarDigest
GZ_TAR_SHA = "4ac76077f2c741c856a2419dfdb0804b18e48d2e1a9ce9c6a3f0605a2078caba"    # its gunzip


def test_reference_gzip_layer_blob(tmp_path):
    """The reference's stored layer blob (lib/utils/testutil/constants.go:28): listed through the
    streaming inflate, inflated with both digests, and equal to the plain-tar fixture's listing."""
    gz_fixture, fixture = _reference_fixtures(tmp_path)           # (the blob is a gzip despite its name: test_layer.tar)
    gz = M.tar_entries(gz_fixture)
    plain = M.tar_entries(fixture)
    assert len(gz) == len(plain) == 390
    assert gz == plain                                      # same entries, same uncompressed offsets
    out = str(tmp_path / "layer.tar")
    r = M.tar_inflate(gz_fixture, out)
    assert r["blob_digest"].hex() == GZ_BLOB_SHA and r["tar_digest"].hex() == GZ_TAR_SHA
    assert r["tar_bytes"] == os.path.getsize(out) == os.path.getsize(fixture)
    assert open(out, "rb").read() == open(fixture, "rb").read()
    assert M.tar_inflate(gz_fixture)["tar_digest"].hex() == GZ_TAR_SHA      # digests only


def test_gzip_layer_roundtrip_and_errors(tmp_path):
    import gzip as gz
    blobs = {"a/b.txt": os.urandom(70000), "a/empty": b"", "c": b"x" * 513}
    p = str(tmp_path / "l.tar")
    with tarfile.open(p, "w", format=tarfile.PAX_FORMAT) as tf:
        ti = tarfile.TarInfo("a/"); ti.type = tarfile.DIRTYPE; tf.addfile(ti)
        for name, data in blobs.items():
            ti = tarfile.TarInfo(name); ti.size = len(data); tf.addfile(ti, io.BytesIO(data))
    raw = open(p, "rb").read()
    pz = str(tmp_path / "l.tar.gz")
    with open(pz, "wb") as f:                               # two gzip members back to back (RFC 1952)
        f.write(gz.compress(raw[:5000]) + gz.compress(raw[5000:]))
    assert M.tar_entries(pz) == M.tar_entries(p)
    r = M.tar_inflate(pz, str(tmp_path / "back.tar"))
    assert open(tmp_path / "back.tar", "rb").read() == raw
    assert r["tar_digest"].hex() == hashlib.sha256(raw).hexdigest()
    assert r["blob_digest"].hex() == hashlib.sha256(open(pz, "rb").read()).hexdigest()
    r2 = M.tar_inflate(p, str(tmp_path / "copy.tar"))      # a plain tar passes through
    assert r2["tar_digest"].hex() == hashlib.sha256(raw).hexdigest()
    bad = str(tmp_path / "bad.gz")
    with open(bad, "wb") as f:
        f.write(gz.compress(raw)[:-300])                    # truncated stream
    with pytest.raises(M.MiError) as ei:
        M.tar_entries(bad)
    assert "gzip" in str(ei.value)
    # a WELL-FORMED gzip stream around a tar that stops inside a member's data: the same error the
    # plain-tar path gives for that archive (the gzip path used to list it without a word)
    cut = raw[: 512 + 512 + 30000]                          # dir header, a/b.txt's header, part of its data
    assert b"a/b.txt" in cut[512:1024]
    open(tmp_path / "cut.tar", "wb").write(cut)
    open(tmp_path / "cut.tar.gz", "wb").write(gz.compress(cut))
    for name in ("cut.tar", "cut.tar.gz"):
        with pytest.raises(M.MiError) as ei:
            M.tar_entries(str(tmp_path / name))
        assert ei.value.code == -1 and "a/b.txt runs past the end of the archive" in str(ei.value), name
    with pytest.raises(M.MiError) as ei:
        M.tar_entries(str(tmp_path / "missing.tar"))
    assert ei.value.code == -5 and "missing.tar" in str(ei.value)


def _e(relpath, kind, **kw):
    d = {"relpath": relpath, "kind": kind, "mode": 0o755 if kind == 0 else 0o644, "mtime_sec": 100, "size": 0}
    d.update(kw)
    return d


def test_apply_layer_filter_drops_what_the_scan_walk_skips(tmp_path):
    """base-image entries the SCAN walk never reports (blacklist, special files, AUFS
    metadata) must not enter the tree, or mi_snapshot_diff writes whiteouts for them."""
    root = str(tmp_path / "rootfs")
    os.makedirs(root)                                          # NewMemFS stats its root
    layer = [_e("bin", 0), _e("bin/sh", 1, size=10), _e("proc", 0), _e("proc/cpuinfo", 1, size=1),
             _e("dev", 0), _e("dev/null", 4, mode=0o666), _e(".wh..wh.plnk", 0), _e(".wh..wh.plnk/x", 1),
             _e("etc", 0), _e("etc/passwd", 1, size=5), _e("var/.wh..wh.opq", 1)]
    merged = M.apply_layer([], layer, root=root, blacklist=[root + "/proc"])
    # (".wh..wh.plnk/x" stays: shouldSkip looks at the BASE name only, utils.go:38 -- the reference keeps it too,
    # creating the skipped parent directory for it on the way: maybeAddToLayer -> addAncestors, mem_fs.go:455-458)
    assert [m["relpath"] for m in merged] == [".wh..wh.plnk", ".wh..wh.plnk/x", "bin", "bin/sh", "dev", "etc", "etc/passwd"]
    # without a blacklist /proc stays; special files and AUFS metadata are skipped whatever the root (shouldSkip), and a
    # special file recurring in a later layer does not abort the merge
    plain = M.apply_layer([], layer)
    assert [m["relpath"] for m in plain] == [".wh..wh.plnk", ".wh..wh.plnk/x", "bin", "bin/sh", "dev", "etc", "etc/passwd", "proc",
                                             "proc/cpuinfo"]
    drop_src = lambda es: [{k: v for k, v in e.items() if k != "src"} for e in es]                   # noqa: E731
    assert drop_src(M.apply_layer(plain, [_e("dev/null", 4, mode=0o600)])) == drop_src(plain)


def test_hard_links_are_applied_after_everything_else():
    base = [_e("a", 0), _e("a/f", 1, size=3), _e("a/h", 3, link_target="a/f")]
    # stream order: the link first, then a whiteout of the same name -- the reference's second pass
    # re-adds the link after the whiteout removed the old one (mem_fs.go:219-236)
    layer = [_e("a/h", 3, link_target="/a/f", mtime_sec=200), _e("a/.wh.h", 1)]
    merged = M.apply_layer(base, layer)
    h = [m for m in merged if m["relpath"] == "a/h"]
    assert len(h) == 1 and h[0]["mtime_sec"] == 200
    # the same link written as bin/x, ./bin/x and /bin/x is ONE target (AbsPath, mem_fs.go:214-216)
    for other in ("/a/f", "./a/f", "a//f"):
        assert M.entry_similar(base[2], dict(base[2], link_target=other))
    assert not M.entry_similar(base[2], dict(base[2], link_target="a/g"))
    same = M.apply_layer(base, [dict(base[2], link_target="/a/f")])
    assert [m for m in same if m["relpath"] == "a/h"][0]["link_target"] == "/a/f"     # (stored as AbsPath, mem_fs.go:214-216)
    assert [m for m in same if m["relpath"] == "a/h"][0]["mtime_sec"] == 100          # similar: the OLD entry stays


def test_snapshot_diff_asks_the_disk_before_writing_a_whiteout(tmp_path):
    """memFSNode.isOnDisk (mem_fs.go:49-57,466) -- a path that still exists but
    is now skipped by the walk gets no whiteout; a path that is really gone gets one."""
    root = tmp_path / "rootfs"
    (root / "data").mkdir(parents=True)
    (root / "mnt").mkdir()
    (root / "data" / "keep").write_bytes(b"k")
    (root / "data" / "gone").write_bytes(b"g")
    (root / "mnt" / "x").write_bytes(b"x")
    before = M.tree_walk(str(root), None, (), M.TREE_SCAN, full=True)
    os.unlink(root / "data" / "gone")
    after = M.tree_walk(str(root), None, [str(root / "mnt")], M.TREE_SCAN, full=True)   # mnt is skipped now
    names = [e["relpath"] for e in before]
    _, wh = M.snapshot_diff(before, after, ignore_time=True)
    assert {names[i] for i, w in enumerate(wh) if w} == {"data/gone", "mnt"}            # entry lists alone
    _, wh = M.snapshot_diff(before, after, ignore_time=True, disk_root=str(root))
    assert {names[i] for i, w in enumerate(wh) if w} == {"data/gone"}                   # the reference's answer


def test_update_mem_fs_cases_replayed():
    """lib/snapshot/mem_fs_test.go:164-344 (TestUpdateMemFS): Simple, Mutation, TrailingSlashes, WhiteoutExistingDir,
    WhiteoutNonexistentNotCausingError -- one layer after another into the tree (makisu_amd.apply_layer: two merges on
    a fresh MemFS handle)."""
    def names(x):
        return sorted("/" + e["relpath"].strip("/") for e in x)
    D = lambda p, mode=0o755: _e(p, 0, mode=0o40000 | mode)                    # noqa: E731
    F = lambda p, mode=0o755: _e(p, 1, mode=0o100000 | mode, size=5)           # noqa: E731
    # Simple
    fs = M.apply_layer(M.apply_layer([], [D("/test1")]), [D("/test1/test2")])
    assert names(fs) == ["/test1", "/test1/test2"]
    # Mutation: the same path again with another mode replaces the node
    fs = M.apply_layer(M.apply_layer([], [F("/test1", 0o755)]), [F("/test1", 0o777)])
    assert names(fs) == ["/test1"] and fs[0]["mode"] & 0o777 == 0o777
    # TrailingSlashes: "test1/" and "test1/test2/" are /test1 and /test1/test2
    fs = M.apply_layer(M.apply_layer([], [D("test1/")]), [D("test1/test2/")])
    assert names(fs) == ["/test1", "/test1/test2"]
    assert names(M.apply_layer(fs, [D("/test1", 0o700)])) == ["/test1", "/test1/test2"]          # one node per path
    # (SkipDirCausesError is a property of the reference's test-only MemFS.merge, testutils_test.go:31-42: the real
    # path, UpdateFromTarReader -> maybeAddToLayer -> addAncestors, creates the missing /test1/test2 instead of failing)
    fs = M.apply_layer([], [D("/test1"), D("/test1/test2/test3")])
    assert names(fs) == ["/test1", "/test1/test2", "/test1/test2/test3"]
    # WhiteoutExistingDir: the subtree goes
    l1 = [D("/test11"), D("/test11/test12"), F("/test11/test12/test.txt")]
    fs = M.apply_layer(M.apply_layer([], l1), [D("/test11"), D("/test11/.wh.test12")])
    assert names(fs) == ["/test11"]
    # WhiteoutNonexistentNotCausingError
    fs = M.apply_layer(M.apply_layer([], l1), [D("/test11"), D("/test11/.wh.test13")])
    assert names(fs) == ["/test11", "/test11/test12", "/test11/test12/test.txt"]
