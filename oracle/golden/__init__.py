"""The generators of tests/golden/: what the imported reference computes, recorded as fixtures.  TEST INFRASTRUCTURE -- never imported by the product; the
reference exists only where fixtures are made, and only the files under tests/golden/ (and the bbfm weight blob) travel with the tests.

    python -m oracle.golden --list              which generator writes which file, and which committed files it reads
    python -m oracle.golden [names...]          regenerate (everything without names), in dependency order
    python -m oracle.golden --check [names...]  regenerate into a temporary directory and compare with the committed files, byte for byte

reference.py finds and patches the reference and holds the shared drivers; registry.py is the table; the other modules hold the generators, by subject.
A new fixture is a function taking (src, dst) in the module of its subject and a row in registry.py.
"""
