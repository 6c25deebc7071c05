/* Empty stand-in for the MSVC header of this name (oracle/ref_nl.mk). */
