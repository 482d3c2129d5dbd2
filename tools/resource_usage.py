#!/usr/bin/env python3
"""Print VGPR / AGPR / SGPR / spills / scratch / occupancy per kernel from hipcc -Rpass-analysis=kernel-resource-usage output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import benchlib

for row in benchlib.usage_rows(open(sys.argv[1]).read()):
    print(row)
