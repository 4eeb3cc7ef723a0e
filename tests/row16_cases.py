"""Hand-built dpkg-grammar tables and installed versions for the 16-byte hot rows (csrc/common.h
Row16 / row16_*; no GPU import here: the host test and the GPU test share this data).

A dpkg key's slot holds the common prefix of its bounds' sort keys (P <= 7 bytes) and a hot row
the 11 key bytes behind it; a pair is decided by the prefix, by the window, or - a window tie with
both keys longer - by the full 32-byte row.  The keys below are named after the case they hold.
"""
import json

DEB, UBU, AMZ = "debian 12", "ubuntu 22.04", "amazon linux 2"
P_CAP, WINDOW = 7, 11
LONG = "1.2.3+" + ".".join(str(i) for i in range(30)) + "-1"  # past the fast encoder's key cap: generic path, spilled key
LONG_LO = LONG.replace("28.29", "28.28")
LONG_HI = LONG.replace("28.29", "28.30")
BAD = "not-a-version"

# key -> fixed versions in advisory order ("" = unfixed, BAD = unparsable)
KEYS = {
    "p0-epochs": ["1:1.0-1", "2.0-1"],                    # the bounds share no byte: P = 0
    "p0-unfixed": [""],                                   # one row and no bound: P = 0
    "p2-majors": ["1.2.3-1", "2.0-1", ""],                # 00 04 | 01 / 02
    "p5-minors": ["1.2-1", "1.10-1"],                     # 00 04 01 ae 04 | 02 / 0a
    "p7-capped": ["1.2.3-1", "1.2.3-2", "1.2.3-1+deb12u1", ""],  # 11 common bytes, capped at 7
    "one-short": ["1", ""],                               # one bound of 6 key bytes: the bound is the prefix
    "one-bound": ["1.2.3-4"],                             # one bound of 13 key bytes: P = 7, 6 in the window
    "beyond": ["1.2.3-1ubuntu0.1", "1.2.3-1ubuntu0.3"],   # 23-byte keys that differ at byte 21: past P + 11
    "zero-bytes": ["256.0-1", "256.512-1", "0:256.256-1"],  # 0x00 key bytes: epoch 0, numbers >= 256
    "long-spill": [LONG],
    "bad-fixed": ["1.0-1", BAD, "2.0-1"],                 # the unparsable bound has no row (Amazon: nor "" )
    "n" * 31: ["1.5-1"], "m" * 32: ["1.5-1"], "k" * 33: ["1.5-1"], "j" * 40: ["1.5-1"], "i" * 41: ["1.5-1"],
}
# absent names of the same lengths: the long ones differ from a present name behind byte 32 only
ABSENT = ["n" * 30 + "x", "m" * 31 + "x", "k" * 32 + "x", "j" * 39 + "x", "i" * 40 + "x", "i" * 33 + "x" * 8, "absent"]

INSTALLED = [
    "0.5", "1", "1.1", "1.2-1", "1.2-2", "1.9-1", "1.10-1", "1.10-2", "1.2.3", "1.2.3-1", "1.2.3-2", "1.2.3-3", "1.2.3-4",
    "1.2.3-5", "1.2.3-1+deb12u1", "1.2.3-1+deb12u2", "1.2.3-1ubuntu0.1", "1.2.3-1ubuntu0.2", "1.2.3-1ubuntu0.3",
    "1.2.3-1ubuntu0.4", "1.2.4-1", "1.5-1", "1.5-2", "2", "2.0-1", "2.0-2", "3.0-1", "1:0.1", "1:1.0-1", "1:1.0-2",
    "2:0.1", "255.9-1", "256.0-1", "256.0-2", "256.256-1", "256.511-9", "256.512-1", "256.513-1", "257", "0:256.0-1",
    LONG_LO, LONG, LONG_HI, BAD, "x1.0",
]


def _rec(path, val):
    return {"path": list(path), "value": val if isinstance(val, str) else json.dumps(val)}


def vuln_id(j):
    return f"CVE-2024-{1000 + j}"


def records():
    recs = [_rec(("data-source", b), {"ID": b.split()[0], "Name": b, "URL": "https://x"}) for b in (DEB, UBU, AMZ)]
    for b in (DEB, UBU, AMZ):
        for key, fixed in KEYS.items():
            for j, f in enumerate(fixed):
                recs.append(_rec((b, key, vuln_id(j)), {"FixedVersion": f}))
    return recs


def packages():
    """Driver package dicts: every key and absent name x every installed version (ID p<i>)."""
    out = []
    for name in list(KEYS) + ABSENT:
        for v in INSTALLED:
            out.append({"ID": f"p{len(out)}", "Name": name, "SrcName": name, "Version": v, "SrcVersion": v})
    return out


def version_key(text):
    """The dpkg sort key of a version (tvm_version_key: the encoder of flattener and kernel), None
    when it does not parse."""
    import ctypes

    from trivy_amd._lib import lib
    buf = (ctypes.c_uint8 * 1024)()
    b = text.encode()
    n = lib().tvm_version_key(1, b, len(b), buf, len(buf))
    return None if n < 0 else bytes(buf[:n])


def has_row(bucket, fixed):
    """debian.go / ubuntu.go: unfixed is a row, an unparsable fixed version none; amazon.go: the
    fixed version must parse ("" does not)."""
    if fixed == "":
        return bucket != AMZ
    return version_key(fixed) is not None
