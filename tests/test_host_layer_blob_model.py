"""CPU tests around the layer-blob add that need no device: the model of the header-candidate rule
(layer_blob_cases.marked_blocks) against blocks pinned by hand, one per clause of the rule, each with a one-byte change that flips the
verdict; two deliberately wrong models that the planted inputs tell from the right one; the prototypes in the header and in the
bindings; the refusals that never reach a device."""
import ctypes as C
import os
import re
import sys
import tarfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import layer_blob_cases as lc  # noqa: E402

H, B = lc.HEADER, lc.BODY


def _flip(block, at, to=None):
    b = bytearray(block)
    b[at] = (b[at] ^ 1) if to is None else to
    return bytes(b)


def test_number_reads_the_field_as_the_text_says():
    for field, want in ((b"0001234\x00", 0o1234), (b"001234\x00 ", 0o1234), (b"  1234  ", 0o1234), (b"\x00\x001234\x00\x00", 0o1234),
                        (b" 12\x0034 ", 0o12),                  # cut at the first NUL behind the trimming
                        (b"        ", 0), (b"\x00" * 8, 0), (b"12345678", None), (b"1234 567", None), (b"-1234567", None),
                        (b"77777777", 0o77777777),
                        (b"\x80\x00\x00\x00\x00\x00\x12\x34", 0x1234), (b"\x80" + b"\xff" * 7, (1 << 56) - 1),
                        (b"\xff" * 8, -1), (b"\xff" * 7 + b"\xfe", -2), (b"\xc0" + b"\x00" * 7, -(1 << 62))):
        assert lc.number(field) == want, (field, lc.number(field), want)


def test_every_clause_of_the_rule_on_a_pinned_block_and_the_byte_that_flips_it():
    plain = lc.raw_header("a/file", 10)
    assert plain[148:156] == b"%06o\x00 " % sum(plain[:148] + b" " * 8 + plain[156:])
    assert lc.is_header(plain)
    # the field's own bytes are counted as spaces, every other byte counts
    for at in (0, 99, 147, 156, 157, 511):
        assert not lc.is_header(_flip(plain, at)), at
    assert not lc.is_header(_flip(plain, 150))                           # a digit of the field: another value
    assert not lc.is_header(_flip(plain, 150, ord("8")))                 # a character that is no octal digit
    assert lc.is_header(_flip(plain, 155, 0)) and lc.is_header(_flip(plain, 154, ord(" ")))   # the padding behind is trimmed either way
    # every form of the field holds, and one bit of its value breaks it
    for form, (field, signed) in lc.CHECKSUM_FORMS.items():
        name = b"n\xff\xfe\x80" if signed else b"name"
        blk = lc.raw_header(name, 3, chksum=field, signed=signed)
        assert lc.is_header(blk), form
        digit = 155 if form in ("base-256", "eight digits", "spaces in front", "NULs in front") else 153
        assert not lc.is_header(_flip(blk, digit)), form
    # the signed sum: only a block with bytes >= 0x80 tells the two sums apart
    signed = lc.raw_header(b"\xc3\xa9", 0, signed=True)
    assert lc.is_header(signed) and not lc.is_header_forgets_signed(signed)
    assert lc.is_header(lc.raw_header(b"\xc3\xa9", 0)) and lc.is_header_forgets_signed(lc.raw_header(b"\xc3\xa9", 0))
    # an empty field is 0: no block of spaces-for-the-field sums to 0, so the zero block is no header; base-256 may be negative
    assert not lc.is_header(bytes(512)) and not lc.is_header(b" " * 512)
    many_high = bytearray(b"\xff" * 512)                                   # unsigned 8*32 + 504*255, signed 256 - 504
    many_high[148:156] = b"\xff" * 7 + bytes((256 - 248,))                  # base-256, complemented: -248
    assert 256 - 504 == -248 and lc.is_header(bytes(many_high)) and not lc.is_header_forgets_signed(bytes(many_high))
    assert not lc.is_header(_flip(bytes(many_high), 155))


def test_blocks_bodies_and_the_trailing_piece():
    x = lc.raw_header("PaxHeaders/f", 30, typeflag=b"x")
    data = b"\x01" * 512
    assert lc.marked_blocks(x + data * 3) == [(0, H), (1, B), (2, B)]
    assert lc.marked_blocks(x + data) == [(0, H), (1, B)] and lc.marked_blocks(data * 2 + x) == [(2, H)]
    assert lc.marked_blocks(x + x + data * 2) == [(0, H), (1, H | B), (2, B), (3, B)]
    for t in b"gLK":
        assert lc.marked_blocks(lc.raw_header("m", 5, typeflag=bytes((t,))) + data * 2) == [(0, H), (1, B), (2, B)]
    for t in b"0125\x00SXl":
        assert lc.marked_blocks(lc.raw_header("m", 5, typeflag=bytes((t,))) + data * 2) == [(0, H)]
    plain = lc.raw_header("f", 0)
    assert lc.marked_blocks(plain[:511]) == [] and lc.marked_blocks(plain + plain[:511]) == [(0, H)]
    assert lc.marked_blocks(b"") == [] and lc.marked_blocks(lc.END) == []
    # the wrong model that marks no BODY differs exactly where a meta header stands
    assert lc.marked_blocks_no_body(x + data * 3) == [(0, H)] != lc.marked_blocks(x + data * 3)
    assert lc.marked_blocks_no_body(plain + data) == lc.marked_blocks(plain + data)


def test_the_wrong_models_differ_on_the_planted_tars_and_only_there():
    hand, _ = lc.hand_made_tar()
    assert lc.marked_blocks(hand) != lc.marked_blocks(hand, header=lc.is_header_forgets_signed)      # the signed-sum member
    assert lc.marked_blocks(hand) != lc.marked_blocks_no_body(hand)                                    # the g header
    ustar, _ = lc.tarfile_tar(tarfile.USTAR_FORMAT)
    assert lc.marked_blocks(ustar) == lc.marked_blocks(ustar, header=lc.is_header_forgets_signed) == lc.marked_blocks_no_body(ustar)
    nested, _ = lc.nested_tar()
    assert len(lc.marked_blocks(nested)) == 2 + len(lc.marked_blocks(ustar))                            # the inner headers are candidates too


def test_the_builders_agree_with_tarfile():
    import io
    for fmt in (tarfile.USTAR_FORMAT, tarfile.GNU_FORMAT, tarfile.PAX_FORMAT):
        tar, members = lc.tarfile_tar(fmt, extra=[] if fmt == tarfile.USTAR_FORMAT else [(lc.long_name(1025), b"long")])
        with tarfile.open(fileobj=io.BytesIO(tar)) as tf:
            regs = [m for m in tf.getmembers() if m.isreg()]
            assert [(m.name.encode(), tf.extractfile(m).read()) for m in regs] == members
            live = [m.offset // 512 for m in tf.getmembers()]
        marked = dict(lc.marked_blocks(tar))
        assert all(marked.get(j, 0) & H for j in live)


def test_the_prototypes_stand_in_the_header_and_in_the_bindings(engine_lib):
    import makisu_amd as M
    head = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "makisu_mi.h")).read(), flags=re.S)
    assert re.search(r"MI_BLOCK int mi_batch_add_layer_blob\(mi_batch\* b, const void\* blob, uint64_t n, uint64_t tag_base,\s*"
                     r"mi_tar\*\* listing, uint8_t\* blob_sha256, mi_layer_blob_info\* info\);", head)
    assert re.search(r"MI_BLOCK int mi_batch_add_layer_path\(mi_batch\* b, const char\* blob_path, uint64_t tag_base,\s*"
                     r"mi_tar\*\* listing, uint8_t\* blob_sha256, mi_layer_blob_info\* info\);", head)
    fields = re.search(r"typedef struct \{([^}]*)\} mi_layer_blob_info;", head).group(1)
    names = re.findall(r"\b([a-z_0-9]+)\s*[,;]", fields)
    assert names == [f for f, _ in M.LayerBlobInfo._fields_]
    assert C.sizeof(M.LayerBlobInfo) == 9 * 8 + 8 + 16 + C.sizeof(M.InflateInfo)
    for name in ("mi_batch_add_layer_blob", "mi_batch_add_layer_path"):
        assert name in engine_lib._mi_symbols and hasattr(engine_lib, name)
    assert callable(M.Batch.add_layer_blob) and callable(M.Batch.add_layer_path)
    local = open(os.path.join(ROOT, "makisu_amd", "csrc", "mi_local.h")).read()
    assert "mi_inflater_run_device" in local and "mi_tar_open_device" in local
    nm = os.popen("nm -D --defined-only " + os.path.join(ROOT, "makisu_amd", "libmakisu_mi.so")).read()
    assert "mi_inflater_run_device" not in nm and "mi_tar_open_device" not in nm        # hidden: not part of the ABI


def test_the_refusals_that_need_no_device(engine_lib):
    blob, sha, info = b"x" * 512, (C.c_uint8 * 32)(), None
    h = C.c_void_p(0xDEAD)
    assert engine_lib.mi_batch_add_layer_blob(None, blob, len(blob), 0, C.byref(h), sha, info) == -1 and h.value is None
    h = C.c_void_p(0xDEAD)
    assert engine_lib.mi_batch_add_layer_path(None, b"/nonexistent", 0, C.byref(h), sha, info) == -1 and h.value is None
    assert engine_lib.mi_batch_add_layer_blob(None, None, 0, 0, None, None, None) == -1
