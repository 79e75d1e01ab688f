"""The model and the builders behind the layer-blob tests: marked_blocks() is the device's header-candidate rule in
plain Python, written from the rule's text with a number() of its own; the builders make tars through tarfile (USTAR, GNU, PAX) and
by hand for what tarfile will not write (a v7 header without magic, a signed-sum checksum, a base-256 checksum field, a field padded
with NULs or spaces at either end, a `g` header), and the gzip forms of a tar."""
import gzip
import io
import tarfile

HEADER, BODY = 1, 2
META_INLINE = 2
META_TYPES = b"xgLK"


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def number(field):
    """a numeric field: base-256 if the top bit of its first byte is set (big-endian, the flag bit dropped, complemented if bit 6 is
    set; more than 63 bits fail), else octal text -- spaces and NULs trimmed on both sides, cut at the first NUL, empty is 0, any
    other character or more than 63 bits fail.  -> the value, or None"""
    if field and field[0] & 0x80:
        inv = 0xFF if field[0] & 0x40 else 0
        x = 0
        for i, c in enumerate(field):
            c ^= inv
            if i == 0:
                c &= 0x7F
            if x >> 56:
                return None
            x = x << 8 | c
        if x >> 63:
            return None
        return -1 - x if inv else x
    t = field.strip(b" \x00")
    t = t.split(b"\x00")[0]
    v = 0
    for c in t:
        if not 0x30 <= c <= 0x37 or v >> 61:
            return None
        v = v << 3 | (c - 0x30)
    return v


def is_header(block):
    """the checksum rule over one 512-byte block"""
    want = number(block[148:156])
    if want is None:
        return False
    counted = block[:148] + b" " * 8 + block[156:]
    unsigned = sum(counted)
    signed = unsigned - 256 * sum(1 for c in counted if c >= 0x80)
    return want == unsigned or want == signed


def marked_blocks(tar, header=is_header, meta_inline=META_INLINE):
    """[(block number, kind)] ascending: HEADER where the rule holds, BODY for the meta_inline blocks behind a header of typeflag x, g,
    L or K where they exist; a trailing piece of 1..511 bytes is no block"""
    n = len(tar) // 512
    kind = [0] * n
    for j in range(n):
        b = tar[512 * j:512 * j + 512]
        if header(b):
            kind[j] |= HEADER
            if b[156] in META_TYPES:
                for d in range(1, meta_inline + 1):
                    if j + d < n:
                        kind[j + d] |= BODY
    return [(j, k) for j, k in enumerate(kind) if k]


# two deliberately wrong models: the planted inputs must tell them from the right one
def is_header_forgets_signed(block):
    want = number(block[148:156])
    return want is not None and want == sum(block[:148] + b" " * 8 + block[156:])


def marked_blocks_no_body(tar):
    return marked_blocks(tar, meta_inline=0)


# ---- headers by hand --------------------------------------------------------------------------------------------------------------------
def raw_header(name, size=0, typeflag=b"0", magic=b"ustar\x0000", chksum=None, signed=False, link=b"", mode=0o644, mtime=1500000000):
    """one 512-byte header; chksum: a function of the sum -> the 8 field bytes (None: "%06o\\0 ", what everybody writes);
    signed: the sum counts bytes >= 0x80 as negative"""
    name = name if isinstance(name, bytes) else name.encode()
    h = bytearray(512)
    h[0:len(name)] = name[:100]
    h[100:108] = b"%07o\x00" % mode
    h[108:116] = b"%07o\x00" % 0
    h[116:124] = b"%07o\x00" % 0
    h[124:136] = b"%011o\x00" % size
    h[136:148] = b"%011o\x00" % mtime
    h[148:156] = b" " * 8
    h[156:157] = typeflag
    h[157:157 + len(link)] = link[:100]
    h[257:257 + len(magic)] = magic
    s = sum(h)
    if signed:
        s -= 256 * sum(1 for c in h if c >= 0x80)
    field = (b"%06o\x00 " % s) if chksum is None else chksum(s)
    assert len(field) == 8
    h[148:156] = field
    return bytes(h)


def pad(data):
    return data + bytes(-len(data) % 512)


def member(name, data, **kw):
    return raw_header(name, len(data), **kw) + pad(data)


END = bytes(1024)

# every form of the checksum field: name -> (the field's writer, signed sum?)
CHECKSUM_FORMS = {
    "usual": (None, False),
    "signed sum": (None, True),
    "base-256": (lambda s: b"\x80" + s.to_bytes(7, "big"), False),
    "NULs in front": (lambda s: b"\x00\x00%06o" % s, False),
    "spaces in front": (lambda s: b"  %06o" % s, False),
    "NULs behind": (lambda s: b"%06o\x00\x00" % s, False),
    "spaces behind": (lambda s: b"%06o  " % s, False),
    "eight digits": (lambda s: b"%08o" % s, False),
}


def hand_made_tar():
    """a tar of hand-made headers only: a v7 header without magic, every form of the checksum field (the signed sum over a name with
    bytes >= 0x80), a `g` header in front of a member -> (tar bytes, [(name, data)] of its regular members)"""
    out, members = b"", []
    data = b"v7 data" * 11
    out += member("v7-no-magic", data, magic=b"")
    members.append(("v7-no-magic", data))
    for i, (form, (field, signed)) in enumerate(sorted(CHECKSUM_FORMS.items())):
        name = ("f%d-" % i).encode() + (b"\xc3\xa9\xff\xfe" if signed else b"") + form.replace(" ", "_").encode()
        data = (form * (i + 3)).encode()
        out += member(name, data, chksum=field, signed=signed)
        members.append((name, data))
    rec = b"19 comment=global!\n"
    out += raw_header("pax_global_header", len(rec), typeflag=b"g") + pad(rec)
    out += member("after-g", b"x" * 513)
    members.append((b"after-g", b"x" * 513))
    return out + END, [(n if isinstance(n, bytes) else n.encode(), d) for n, d in members]


# ---- tars through tarfile ---------------------------------------------------------------------------------------------------------------
SIZES = (0, 1, 511, 512, 513, 70000)


def content(n, seed):
    """n bytes that compress, differ by seed and repeat nowhere across members"""
    out = bytearray()
    x = seed * 2654435761 % (1 << 32) or 1
    while len(out) < n:
        x = x * 1103515245 + 12345 & 0xFFFFFFFF
        out += b"%08x-%d " % (x, seed) * (1 + (x >> 28))
    return bytes(out[:n])


def tarfile_tar(fmt, extra=(), end_marker=True):
    """regular members of SIZES with a directory, a symlink and a hard link in between, in one of tarfile's formats; extra: further
    (name, data) members -> (tar bytes, [(name, data)] of the regular members in order)"""
    buf = io.BytesIO()
    members = []
    with tarfile.open(fileobj=buf, mode="w", format=fmt) as tf:
        def add(name, data=None, type_=tarfile.REGTYPE, link=""):
            ti = tarfile.TarInfo(name)
            ti.type, ti.linkname, ti.mtime, ti.mode = type_, link, 1500000000, 0o755 if type_ == tarfile.DIRTYPE else 0o644
            ti.size = len(data) if data is not None else 0
            tf.addfile(ti, io.BytesIO(data) if data is not None else None)
            if data is not None:
                members.append((name.encode(), data))
        add("dir", type_=tarfile.DIRTYPE)
        for i, n in enumerate(SIZES):
            add("dir/file-%d" % n, content(n, i + 1))
            if i == 1:
                add("dir/sym", type_=tarfile.SYMTYPE, link="file-1")
            if i == 3:
                add("dir/hard", type_=tarfile.LNKTYPE, link="dir/file-1")
                add("dir/sub", type_=tarfile.DIRTYPE)
        for name, data in extra:
            add(name, data)
    tar = buf.getvalue()
    if not end_marker:
        tar = tar.rstrip(b"\x00")
        tar += bytes(-len(tar) % 512)
        # (a member's own trailing zero bytes went with the marker: every member here ends in a non-zero byte or is padded back)
    return tar, members


def long_name(n):
    return ("d/" + "n" * (n - 2))[:n]


def nested_tar():
    """a tar whose one large member is itself a tar: its inner headers are dead candidates"""
    inner, _ = tarfile_tar(tarfile.USTAR_FORMAT)
    return member("inner.tar", inner) + member("tail", b"tail") + END, [(b"inner.tar", inner), (b"tail", b"tail")]


def pax_size_override():
    """an `x` header whose size record overrides the member's own size field (which says 0)"""
    data = content(1500, 77)
    rec_body = b" size=%d\n" % len(data)
    n = len(rec_body) + 2
    rec = b"%d%s" % (n, rec_body)
    assert len(rec) == n
    tar = raw_header("PaxHeaders/overridden", len(rec), typeflag=b"x") + pad(rec)
    tar += raw_header("overridden", 0) + pad(data) + END
    return tar, [(b"overridden", data)]


# ---- the gzip forms ---------------------------------------------------------------------------------------------------------------------
def foreign_gzip(tar):
    """one zlib stream, no markers: not parallel"""
    return gzip.compress(tar, 6, mtime=0)
