"""Runs one bench.py leg alone and prints its JSON: python tools/leg.py live_path [cpu]."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
name = sys.argv[1]
cpu = len(sys.argv) > 2 and sys.argv[2] == "cpu"
fn = getattr(bench, name + "_leg")
steps = {"tracker": 20, "matcher": 50}  # the legs that take a step count
out = fn(0, steps[name], cpu) if name in steps else fn(0, cpu)
print(json.dumps(out, indent=1))
