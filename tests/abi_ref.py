"""What the public headers declare, for the tests of the C ABI's Python binding."""
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def declared_symbols(header):
    """The t2h_* functions the public header ``header`` (a name under include/, or a path to it) declares, comments stripped."""
    text = open(os.path.join(INCLUDE, os.path.basename(header))).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(t2h_[a-z0-9_]+)\s*\(", text)))
