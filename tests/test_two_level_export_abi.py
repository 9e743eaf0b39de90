"""art_export_two_level without a GPU: declared and exported, ArtTwoLevelInfo / ArtTwoLevelBuffers match the header, and a call without
a scene is refused before anything touches a device."""
import ctypes as C
import os
import re


def test_the_symbol_is_declared_and_exported_and_the_structs_match_the_header(art):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(art.ROOT, "include", "art_hip.h")).read(), flags=re.S)
    L = art.load_library()
    assert re.search(r"int\s+art_export_two_level\(ArtTwoLevelInfo\* info, const ArtTwoLevelBuffers\* buf\);", hdr)
    assert "art_export_two_level" in art.EXPORTED_SYMBOLS and L.art_export_two_level is not None
    rec = re.search(r"typedef struct ArtTwoLevelInfo \{(.*?)\} ArtTwoLevelInfo;", hdr, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"\b(int32_t|float)\b", "", rec.group(1)))
    I = art.ArtTwoLevelInfo
    assert names == [n for n, _ in I._fields_]
    assert C.sizeof(I) == 56 and [t for _, t in I._fields_] == [C.c_int32] * 8 + [C.c_float] * 5 + [C.c_int32]
    rec = re.search(r"typedef struct ArtTwoLevelBuffers \{(.*?)\} ArtTwoLevelBuffers;", hdr, flags=re.S)
    ptrs = re.findall(r"\*\s*(\w+)\s*;", rec.group(1))
    B = art.ArtTwoLevelBuffers
    assert tuple(ptrs) == art.TWO_LEVEL_ARRAYS and [n for n, _ in B._fields_] == ptrs + ["cap"]
    assert re.search(r"int64_t cap\[10\];", rec.group(1)) and C.sizeof(B) == 10 * 8 + 10 * 8 and B.cap.offset == 80
    assert L.art_export_two_level.argtypes == [C.POINTER(I), C.POINTER(B)]


def test_an_export_without_a_scene_is_refused(art):
    L = art.load_library()
    info = art.ArtTwoLevelInfo()
    assert L.art_export_two_level(None, None) != 0
    assert "art_export_two_level: null ArtTwoLevelInfo" in L.art_last_error().decode()
    assert L.art_export_two_level(C.byref(info), None) != 0
    assert "art_export_two_level: no scene uploaded" in L.art_last_error().decode()
    out, rc = art.two_level_arrays(L.art_export_two_level)
    assert out is None and rc != 0
