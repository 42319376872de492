"""Hand-made EXIF APP1 segments and JPEG files that carry them, for the tests of mjh_exif_orientation and the oriented tensor output."""
import struct


def tiff(orientation=None, le=True, entries=None, ifd1=None, ifd_off=8, count=None):
    """A TIFF block: header, IFD0 with `entries` ((tag, type, count, value) tuples; by default one Orientation SHORT) and, when ifd1 is
    given, an IFD1 holding those entries.  count overrides IFD0's entry count."""
    e = "<" if le else ">"
    if entries is None:
        entries = [] if orientation is None else [(0x0112, 3, 1, orientation)]
    hdr = (b"II*\0" if le else b"MM\0*") + struct.pack(e + "I", ifd_off)
    body = bytearray(hdr + b"\0" * (ifd_off - 8))

    def ifd(ents, nxt):
        b = struct.pack(e + "H", len(ents) if count is None or ents is not entries else count)
        for tag, typ, cnt, val in ents:
            v = struct.pack(e + "H", val & 0xFFFF) + b"\0\0" if typ == 3 else struct.pack(e + "I", val & 0xFFFFFFFF)
            b += struct.pack(e + "HHI", tag, typ, cnt) + v
        return b + struct.pack(e + "I", nxt)

    ifd0_len = 2 + 12 * len(entries) + 4
    nxt = ifd_off + ifd0_len if ifd1 is not None else 0
    body += ifd(entries, nxt)
    if ifd1 is not None:
        body += ifd(ifd1, 0)
    return bytes(body)


def app1(payload, exif=True):
    """an APP1 segment around payload (after 'Exif\\0\\0' when exif)"""
    p = (b"Exif\0\0" if exif else b"") + payload
    return b"\xff\xe1" + struct.pack(">H", len(p) + 2) + p


def insert(jpeg, *segments, after_sof=False):
    """jpeg with the segments put right after SOI (or right after the SOF segment)"""
    jpeg = bytes(jpeg)
    at = 2
    if after_sof:
        i = 2
        while True:
            m, ln = jpeg[i + 1], struct.unpack(">H", jpeg[i + 2:i + 4])[0]
            i += 2 + ln
            if m in (0xC0, 0xC1, 0xC2):
                at = i
                break
    return jpeg[:at] + b"".join(segments) + jpeg[at:]


def tagged(jpeg, orientation, le=True):
    """jpeg carrying an Exif APP1 with the given Orientation"""
    return insert(jpeg, app1(tiff(orientation, le)))
