"""Generates tests/golden/finder_bytes.json: for every case below — the smallest settings and input that reach one instance of the
match finder's kernels (zstdsharp_amd/csrc/lz_fast.hip: launch_lz picks it, resolve_framing and launch_state in zstd_mi355x.hip decide
what it is picked from) — the sizes and the SHA-256 of what this project's own encoder writes.  The file holds no compressed data.
Run on a machine with an MI355X and the built library:  python tests/golden/make_finder_bytes.py
Before anything is recorded every output is decoded, written a second time, and checked to have taken the path the case was written
for (check_path).  tests/test_gpu_finder_bytes.py runs the same cases through the same functions and compares."""
import ctypes, hashlib, io, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import datagen

JSON_PATH = os.path.join(HERE, "finder_bytes.json")
ZSTD_c_windowLog = 101
KiB = 1 << 10
RAND_DICT = ["gen", "rand", 112640, 4242]          # rand_dict() of tests/test_gpu_dict_index.py: its only redundancy is itself
RAW_DICT = ["file", "rawcontent_6000.dict"]
REGION, TILES = "region", "tiles"


# input: a list of entries (one, unless the call is a batch), each a list of pieces: [kind, n, seed] = datagen.gen(kind, n, seed), or
# ["dict", a, n] = n bytes of the case's dictionary from a (negative: from its end).
# region_kernel: the call's last pass launches lz_region_kernel, so its stage names hold "lz_region" (they do whether or not a chunk
# was listed for it; the fast and the dual finder behind LDS history, and the dual finder everywhere, run the region parse inside lz_kernel).
# parse: REGION = some chunk's parse leaves the tile loop for the region parse, TILES = none does.  The stage names cannot tell, the
# bytes can: ZSTDMI_CCtx_setParser(1) keeps every chunk in the tile loop, and the case writes other bytes under it exactly if REGION.
def case(name, level, entries, region_kernel, parse, **settings):
    return dict(name=name, level=level, settings=settings, input=entries, region_kernel=region_kernel, parse=parse)


def cases(cus):
    batch = [[["text", 3000, 41]], [["zipf", 20000, 42]], [["text", 150000, 43]], [["rand", 4000, 44]], [["mixed", 150001, 45]], [["text", 30000, 46]]]
    out = []
    # plain chunks, each a frame: lz_kernel<0|1|2,F,F,0>; dense text goes on in lz_region_kernel<0,F,0> / <2,F,0> (the dual finder: inline)
    out += [case(f"plain-text-l{l}", l, [[["text", 60000, 100 + l]]], l != 3, REGION) for l in (1, 3, 5)]
    # ... and input that stays in the tile loop: super-tiles, literals counted and never copied
    out += [case(f"plain-{k}-l1", 1, [[[k, 64 * KiB, 110 + i]]], True, TILES) for i, k in enumerate(("zipf", "rand"))]
    out += [case("parser-off-l1", 1, [[["text", 60000, 101]]], False, TILES, parser=1)]
    # blocks behind LDS history: <0|1|2,T,F,0>, lz_region_kernel<2,T,0>; level 1 writes 64 KiB frames of four 16 KiB blocks
    out += [case(f"history-text-l{l}", l, [[["text", 200000, 120 + l]]], l == 5, REGION) for l in (1, 3, 5)]
    # a prefix that is not part of the input (the record is too short for the region parse: four tiles with the dictionary's two)
    out += [case("rawdict-l1", 1, [[["text", 5000, 130]]], False, TILES, dictionary=RAW_DICT)]
    # independent 4 KiB blocks inside 64 KiB frames: one tile each
    out += [case("window12-l1", 1, [[["text", 100000, 131]]], False, TILES, params=[[ZSTD_c_windowLog, 12]])]
    # full 64 KiB blocks with far candidates: <0,F,T,0>, which has no region parse
    out += [case("far-l1", 1, [[["text", 300000, 132]]], False, TILES, params=[[ZSTD_c_windowLog, 18]])]
    # the table form: <0|1|2,T,F,1>, lz_region_kernel<2,T,1>.  (A pass per group of entries with the same framing and the same
    # resolved parameters, in the order in which the groups first occur: the last pass is the one of the two long entries.)
    out += [case(f"batch-l{l}", l, batch, l == 5, REGION, call="batch") for l in (1, 3, 5)]
    # one frame per call: <0,F,T,2>, <1,T,F,2>, <2,T,F,2>, lz_region_kernel<2,T,2>; and a session cut into two batches
    out += [case(f"single-l{l}", l, [[["text", 300000, 140 + l]]], l == 5, TILES if l == 1 else REGION, single_frame=1) for l in (1, 3, 5)]
    out += [case("single-stream-l3", 3, [[["text", 300000, 150]]], False, REGION, single_frame=1, call="stream", stream_cut=170001)]
    # an indexed dictionary: <0,F,T,3> and, with dict_index_strategy 2, <1,F,T,3>; then a match that runs to the dictionary's end
    mixed = [["dict", 1000, 700], ["rand", 100, 9], ["dict", 45000, 700], ["rand", 100, 10], ["dict", 100000, 700], ["text", 900, 11]]
    tail = [["dict", -300, 300], ["text", 500, 12], ["dict", -40, 40], ["dict", 0, 40]]
    out += [case("dict-index-l1", 1, [mixed], False, TILES, dictionary=RAND_DICT, dict_index=1)]
    out += [case("dict-index-l3", 3, [mixed], False, TILES, dictionary=RAND_DICT, dict_index=1, dict_index_strategy=2)]
    out += [case("dict-index-tail-l1", 1, [tail], False, TILES, dictionary=RAND_DICT, dict_index=1)]
    out += [case("dict-index-tail-l3", 3, [tail], False, TILES, dictionary=RAND_DICT, dict_index=1, dict_index_strategy=2)]
    # more chunks than compute units: the chunks are claimed from a counter and arrive prefetched.  (Who parses a chunk depends on
    # timing; what is written for it does not.)
    out += [case("claimed-l1", 1, [[["mixed", 64 * KiB * (cus + 1), 160]]], True, REGION, history=[0, 0], claims=1)]
    # negative levels: raw literals; from level -6 on a floor under the probing stride (minStrideLog), which has no region parse
    out += [case("negative-l-5", -5, [[["text", 64 * KiB, 161]]], True, REGION)]
    out += [case("negative-l-20", -20, [[["text", 64 * KiB, 162]]], False, TILES)]
    return out


def dictionary_of(c):
    d = c["settings"].get("dictionary")
    if not d:
        return None
    return datagen.gen(d[1], d[2], d[3]) if d[0] == "gen" else open(os.path.join(HERE, d[1]), "rb").read()


def entries_of(c):
    dic = dictionary_of(c)

    def piece(p):
        if p[0] != "dict":
            return datagen.gen(p[0], p[1], p[2])
        a = p[1] if p[1] >= 0 else len(dic) + p[1]
        return dic[a:a + p[2]]
    return [b"".join(piece(p) for p in e) for e in c["input"]]


def stage_names(lib, cctx):
    ms, names = (ctypes.c_float * 24)(), (ctypes.c_char_p * 24)()
    return [names[i].decode() for i in range(lib.ZSTDMI_CCtx_getStageTimes(cctx, ms, names, 24))]


def stream_session(lib, cctx, pieces):
    """ZSTD_compressStream2: a ZSTD_e_flush behind every piece but the last, which goes in with ZSTD_e_end -> bytes"""
    from zstdsharp_amd.errors import get_error_code, is_error
    from zstdsharp_amd.streams import ZSTD_inBuffer, ZSTD_outBuffer, ZSTD_e_end, ZSTD_e_flush
    room, out = ctypes.create_string_buffer(lib.ZSTD_CStreamOutSize()), bytearray()
    for i, p in enumerate(pieces):
        keep = ctypes.create_string_buffer(p, len(p))
        inb = ZSTD_inBuffer(ctypes.addressof(keep), len(p), 0)
        while True:
            ob = ZSTD_outBuffer(ctypes.addressof(room), len(room), 0)
            r = lib.ZSTD_compressStream2(cctx, ctypes.byref(ob), ctypes.byref(inb), ZSTD_e_end if i == len(pieces) - 1 else ZSTD_e_flush)
            assert not is_error(r), get_error_code(r)
            out += room.raw[:ob.pos]
            if r == 0:
                break
    return bytes(out)


def run_case(c, entries, parser=None):
    """-> (what the encoder writes for each entry, the stage names of the call's last pass).  parser: ZSTDMI_CCtx_setParser, over the case's own."""
    import torch
    import zstdsharp_amd as z
    s = c["settings"]
    if s.get("claims"):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert len(entries[0]) > 64 * KiB * cus, f"{c['name']}: {len(entries[0])} bytes are not more chunks than this device's {cus} compute units"
    with z.Compressor(c["level"]) as cz:
        lib = cz._lib
        for p, v in s.get("params", ()):
            cz.SetParameter(p, v)
        if parser is not None or "parser" in s:
            assert lib.ZSTDMI_CCtx_setParser(cz.cctx, s["parser"] if parser is None else parser) == 0
        if "history" in s:
            assert lib.ZSTDMI_CCtx_setHistory(cz.cctx, *s["history"]) == 0
        if "dictionary" in s:
            cz.LoadDictionary(dictionary_of(c))
        if "dict_index" in s:
            cz.dict_index = bool(s["dict_index"])
        if "dict_index_strategy" in s:
            cz.dict_index_strategy = s["dict_index_strategy"]
        if "single_frame" in s:
            cz.single_frame = bool(s["single_frame"])
        assert lib.ZSTDMI_CCtx_setProfiling(cz.cctx, 1) == 0
        call = s.get("call", "wrap")
        if call == "batch":
            outs = z.compress_batch(cz, entries)
        elif call == "stream":
            outs = [stream_session(lib, cz.cctx, [entries[0][:s["stream_cut"]], entries[0][s["stream_cut"]:]])]
        else:
            outs = [cz.Wrap(e) for e in entries]
        return outs, stage_names(lib, cz.cctx)


def check_path(c, outs, names, entries):
    """the case took the path it was written for (see case())"""
    assert ("lz_region" in names) == c["region_kernel"], (c["name"], names)
    tiles_only, _ = run_case(c, entries, parser=1)
    assert (tiles_only != outs) == (c["parse"] == REGION), f"{c['name']}: meant for parse = {c['parse']}, but the tile loop alone writes {'other' if tiles_only != outs else 'the same'} bytes"


def check_roundtrip(c, outs, entries, oracle):
    """the GPU decoder restores every entry; behind a dictionary the oracle's dictionary decoder does too"""
    import zstdsharp_amd as z
    dic = dictionary_of(c)
    with z.Decompressor() as d:
        if dic is not None:
            d.LoadDictionary(dic)
            for o, e in zip(outs, entries):
                assert oracle.decompress(o, len(e), dic) == e, (c["name"], len(e))
        if c["settings"].get("call") == "stream":      # (a session's frame states no content size)
            with z.DecompressionStream(io.BytesIO(outs[0]), decompressor=d) as ds:
                assert ds.ReadToEnd() == entries[0], c["name"]
            return
        back = z.decompress_batch(d, outs, [len(e) for e in entries])
        for b, e in zip(back, entries):
            assert bytes(b) == e, (c["name"], len(e))


def digest(outs):
    return [len(o) for o in outs], hashlib.sha256(b"".join(outs)).hexdigest()


def main():
    import torch
    import oracle_lib
    torch.zeros(1, device="cuda")
    recorded, wrong = [], []
    for c in cases(torch.cuda.get_device_properties(0).multi_processor_count):
        entries = entries_of(c)
        outs, names = run_case(c, entries)
        c["sizes"], c["sha256"] = digest(outs)
        print(c["name"], c["sizes"], c["sha256"][:16], " ".join(names), flush=True)
        try:        # (every case is looked at before the run fails, so that one run shows all there is to mend)
            check_path(c, outs, names, entries)
            check_roundtrip(c, outs, entries, oracle_lib)
            assert run_case(c, entries)[0] == outs, f"{c['name']}: two runs wrote different bytes"
        except AssertionError as e:
            wrong.append(str(e)); print("  WRONG:", e, flush=True)
        recorded.append(c)
    assert not wrong, f"{len(wrong)} case(s) did not do what they were written for: nothing recorded"
    with open(JSON_PATH, "w") as f:
        f.write(json.dumps(dict(generator="tests/golden/make_finder_bytes.py", cases=recorded), indent=1) + "\n")


if __name__ == "__main__":
    main()
