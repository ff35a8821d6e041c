"""Size of the BGZF writer's DEFLATE blocks against zlib level 1: runs the host twin over the three texts of
tests/bgzf_cases.size_texts() and raw DEFLATE at zlib level 1 over the same 65280-byte blocks (what `bgzip -l 1` would write), and records
both totals per text in profiles/r15_bgzf_sizes.json, which tests/test_bgzf.py holds the twin against.  CPU only.

    python tools/bgzf_sizes.py [--out profiles/r15_bgzf_sizes.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_bgzf_sizes.json"))
    a = ap.parse_args()
    import bgzf_cases as BC
    texts = {}
    for name, data in BC.size_texts().items():
        twin, z1 = BC.twin_and_zlib1(data)
        texts[name] = {"raw": len(data), "twin": twin, "zlib1": z1, "twin_over_zlib1": round(twin / z1, 4), "margin": BC.size_margin(twin, z1)}
        print(name, texts[name])
    with open(a.out, "w") as f:
        json.dump({"what": "bytes of DEFLATE blocks over 65280-byte blocks: host twin of mcom_bgzf_encode against zlib level 1 (raw deflate)", "texts": texts}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
